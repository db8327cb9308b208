"""Host-side checks of the "fp16" convolution mode: the config / environment selection and the library's mode switch (argument
validation and the mode query need no GPU)."""
import pytest
import torch


def _cfg(**kw):
    from spatialalignmentnetwork_amd import basemodel
    base = dict(sparsity=0.25, lr=1e-4, shape=64, coils=1, reg="Rec", mask="equispaced", weight_smooth=1000.0, weight_gan=0.0,
                weight_gan_sim=0.0, weight_sim=1.0, use_amp=False, num_cascades=2)
    base.update(kw)
    return basemodel.Config(**base)


def test_environment_default_selects_the_fp16_mode(monkeypatch):
    """SAN_CONV_DTYPE names the mode use_amp selects for a config without conv_dtype (the reference's --use_amp through dropin/):
    with use_amp off (the reference's eval.py after loading) the fp32-equivalent mode stays, and unset nothing changes."""
    from spatialalignmentnetwork_amd import model, ops
    assert "fp16" in ops.CONV_PRECISIONS
    monkeypatch.setenv("SAN_CONV_DTYPE", "fp16")
    net = model.CSModel(_cfg(use_amp=True))
    assert net.conv_dtype is None and net._conv_mode() == "fp16"
    net.use_amp = False                                  # eval.py:41
    assert net._conv_mode() == "bf16x3"
    assert model.CSModel(_cfg())._conv_mode() == "bf16x3"
    # an explicit key wins over the environment
    assert model.CSModel(_cfg(use_amp=True, conv_dtype="bf16x3"))._conv_mode() == "bf16x3"
    monkeypatch.delenv("SAN_CONV_DTYPE")
    for kw, want in ((dict(use_amp=True), "bf16"), (dict(), "bf16x3"), (dict(conv_dtype="fp8"), "fp8")):
        assert model.CSModel(_cfg(**kw))._conv_mode() == want, kw
    assert model.CSModel(_cfg(bwd_dtype="fp16")).bwd_dtype == "fp16"
    monkeypatch.setenv("SAN_CONV_DTYPE", "fp17")
    with pytest.raises(ValueError):
        model.CSModel(_cfg(use_amp=True))


def test_library_mode_switch():
    import __graft_entry__ as ge
    ge.build()
    from spatialalignmentnetwork_amd import ops
    lib = ops.lib()
    try:
        assert ops.set_conv_precision("fp16") == "bf16x3"
        assert lib.query("san_get_conv_precision") == 17 and ops.current_precision() == "fp16"
        assert ops._fwd_fmt() == 64 and ops._grad_fmt() == 64
        assert ops.set_conv_precision("bf16") == "fp16"
        assert lib.query("san_get_conv_precision") == 1 and ops._fwd_fmt() == 0
    finally:
        ops.set_conv_precision("bf16x3")
    with pytest.raises(RuntimeError):
        lib.call("san_set_conv_precision", 16)
