"""The "fp16" convolution mode: one fp16 part per operand, one v_mfma_f32_16x16x32_f16 product per MAC, for the forward, data-gradient
and weight-gradient convolutions."""
import math

import pytest
import torch
import torch.nn.functional as F
from conftest import philox, rel_err, load_golden, as_t  # noqa: F401
from gpu_common import S, g, DEV, _fill, _psnr  # noqa: F401

pytestmark = pytest.mark.gpu


def _pow2_scale(t: torch.Tensor) -> float:
    """The library's power-of-two operand scale: max |t| x S in [2^13, 2^14)."""
    m = float(t.abs().max())
    return 2.0 ** (13 - (math.frexp(m)[1] - 1))


def _q16(t: torch.Tensor, scaled: bool) -> torch.Tensor:
    """t rounded to fp16 once (x its power-of-two scale first when `scaled`), as float64 in t's units."""
    s = _pow2_scale(t) if scaled else 1.0
    return (t.double() * s).half().double() / s


def _grad_act(ops, gout):
    """A dy Act written by the activation backward (identity activation: dy == gout); in the fp16 mode it carries an amax record."""
    n, c, h, w = gout.shape
    ops.AMAX.reset(DEV)
    dy = ops.Act(torch.empty((n, c, h, w), device=DEV), 0, c)
    ops.act_bwd(ops.full(g(gout)), ops.full(g(philox("h1.y", (n, c, h, w)))), dy, instance_norm=False)
    assert (dy.amax is not None) == (ops.current_precision() in ("fp16", "bf16x3"))
    return dy


def _run_three(ops, mode, x, wt, gout, ks):
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    with ops.conv_precision(mode):
        y = torch.empty((n, cout, h, w), device=DEV)
        ops.conv2d(ops.full(g(x)), g(wt), None, ops.full(y))
        dy = _grad_act(ops, gout)
        dx = torch.empty((n, cin, h, w), device=DEV)
        ops.conv2d_dgrad(dy, g(wt), ops.full(dx))
        dw = torch.zeros((cout, cin, ks, ks), device=DEV)
        if ks == 3:
            ops.conv2d_wgrad_bf16x3(ops.full(g(x)), dy, dw)
        else:
            ops.conv2d_wgrad1x1_bf16x3(ops.full(g(x)), dy, dw)
        torch.cuda.synchronize()
    return y.cpu().double(), dx.cpu().double(), dw.cpu().double()


def _ref64(x64, w64, gout64, ks):
    x64 = x64.clone().requires_grad_(True)
    w64 = w64.clone().requires_grad_(True)
    y = F.conv2d(x64, w64, padding=ks // 2)
    (y * gout64).sum().backward()
    return y.detach(), x64.grad, w64.grad


@pytest.mark.parametrize("gscale", [1e-7, 1.0, 1e4])
@pytest.mark.parametrize("n,cin,cout,h,w,ks", [
    (2, 72, 36, 40, 40, 3),        # tiled kernel, FLAT tiles
    (1, 288, 144, 20, 20, 3),      # deep K (split-K)
    (2, 18, 36, 160, 160, 3),      # persistent (stream) kernel, partial channel block
    (1, 36, 18, 320, 320, 3),      # persistent kernel at 320^2
    (1, 24, 16, 160, 160, 3),      # persistent kernel, one full block
    (1, 48, 32, 160, 160, 3),      # persistent kernel, two full blocks (and its data gradient 32 -> 48... -> 32 channels)
    (1, 32, 48, 160, 160, 3),      # persistent kernel, three full blocks
    (2, 64, 96, 32, 48, 1),        # 1x1 one-stage GEMM
])
def test_fp16_one_part_forms_round_each_operand_once(S, n, cin, cout, h, w, ks, gscale):
    """Forward, data gradient and weight gradient of the fp16 mode against float64 on the fp16-rounded operands (weights x S_w,
    gradients x their amax scale): one rounding per operand and nothing else.  Against float64 on the unrounded operands the
    error is at most a quarter of the one-part bf16 form's on the same data."""
    ops = S.ops
    x = philox("h1.x", (n, cin, h, w)) * 2
    wt = philox("h1.w", (cout, cin, ks, ks)) * 0.1
    rng = torch.exp(philox("h1.r", (n, cout, h, w)) * 4.0)
    gout = philox("h1.g", (n, cout, h, w)) * rng * (gscale / rng.max())
    got = _run_three(ops, "fp16", x, wt, gout, ks)
    assert ops.current_precision() == "bf16x3" and ops.lib().query("san_get_conv_precision") == 3
    q = _ref64(_q16(x, False), _q16(wt, True), _q16(gout, True), ks)
    exact = _ref64(x.double(), wt.double(), gout.double(), ks)
    bf = _run_three(ops, "bf16", x, wt, gout, ks)
    for name, a, r, e, b in zip(("forward", "data gradient", "weight gradient"), got, q, exact, bf):
        eq, ee, eb = rel_err(a, r), rel_err(a, e), rel_err(b, e)
        print(f"fp16 {name} {cin}->{cout} k{ks} @{h}x{w} dy~{gscale:g}: vs rounded float64 {eq:.2e}, vs exact {ee:.2e} "
              f"(bf16 {eb:.2e}, ratio {ee / eb:.3f})")
        assert eq <= 1e-6, (name, eq)
        assert ee <= 0.25 * eb, (name, ee, eb)


def test_fp16_transposed_convolution_and_channel_views(S):
    """The transposed 2x2 convolution (pixel-shuffle epilogue of the one-stage GEMM) and a 3x3 layer reading / writing channel views."""
    ops = S.ops
    n, cin, cout, h, w = 2, 72, 36, 40, 40
    x = philox("h1.tx", (n, cin, h, w))
    wt = philox("h1.tw", (cin, cout, 2, 2)) * 0.1
    with ops.conv_precision("fp16"):
        y = torch.empty((n, cout, 2 * h, 2 * w), device=DEV)
        ops.tconv2x2(ops.full(g(x)), g(wt), ops.full(y))
        torch.cuda.synchronize()
    want = F.conv_transpose2d(_q16(x, False), _q16(wt, True), stride=2)
    e = rel_err(y.cpu().double(), want)
    print(f"fp16 transposed 2x2 {cin}->{cout}: {e:.2e}")
    assert e <= 1e-6
    # 3x3 forward from channels 8..80 of a 96-channel tensor into channels 4..40 of a 48-channel one
    xb = philox("h1.vx", (n, 96, h, w))
    wv = philox("h1.vw", (36, 72, 3, 3)) * 0.1
    with ops.conv_precision("fp16"):
        yb = torch.zeros((n, 48, h, w), device=DEV)
        ops.conv2d(ops.Act(g(xb), 8, 72), g(wv), None, ops.Act(yb, 4, 36))
        torch.cuda.synchronize()
    want = F.conv2d(_q16(xb[:, 8:80], False), _q16(wv, True), padding=1)
    e = rel_err(yb[:, 4:40].cpu().double(), want)
    assert e <= 1e-6, e
    assert float(yb[:, :4].abs().max()) == 0.0 and float(yb[:, 40:].abs().max()) == 0.0


@pytest.mark.parametrize("gscale", [1e-7, 1e4])
def test_fp16_few_channel_partial_blocks(S, gscale):
    """The persistent kernel's <0, REM> forms: a forward convolution to 2 channels (32 -> 2 @320^2) and the data gradient of a
    3 -> 18 convolution (18 -> 3 channels)."""
    ops = S.ops
    n, h, w = 1, 320, 320
    x = philox("h1.fx", (n, 32, h, w))
    wt = philox("h1.fw", (2, 32, 3, 3)) * 0.1
    with ops.conv_precision("fp16"):
        y = torch.empty((n, 2, h, w), device=DEV)
        ops.conv2d(ops.full(g(x)), g(wt), None, ops.full(y))
        torch.cuda.synchronize()
    e = rel_err(y.cpu().double(), F.conv2d(_q16(x, False), _q16(wt, True), padding=1))
    assert e <= 1e-6, e
    w3 = philox("h1.f3", (18, 3, 3, 3)) * 0.1
    gout = philox("h1.fg", (n, 18, h, w)) * gscale
    with ops.conv_precision("fp16"):
        dy = _grad_act(ops, gout)
        dx = torch.empty((n, 3, h, w), device=DEV)
        ops.conv2d_dgrad(dy, g(w3), ops.full(dx))
        torch.cuda.synchronize()
    want = torch.nn.grad.conv2d_input((n, 3, h, w), _q16(w3, True), _q16(gout, True), padding=1)
    e = rel_err(dx.cpu().double(), want)
    print(f"fp16 few-channel data gradient dy~{gscale:g}: {e:.2e}")
    assert e <= 1e-6, e


# ------------------------------------------------------------------------------------------- model level
def test_fp16_psnr_on_trained_like_weights(S):
    """The damped weight set of test_narrow_precision_psnr_on_trained_like_weights at N = 8: the fp16 mode's reconstruction
    against the fp32-equivalent one, beside the bf16 mode's in the same run.  Measured: fp16 59.2 dB, bf16 44.9 dB (one fp16
    rounding per operand costs 1/8 of a bf16 one: 3 bits, 18 dB); the bar sits 3 dB below."""
    n, c, h, w = 8, 1, 320, 320
    cfg = S.base.Config(sparsity=0.25, lr=1e-4, shape=w, coils=c, reg="Rec", mask="equispaced", weight_smooth=1000.0,
                        weight_gan=0.0, weight_gan_sim=0.0, weight_sim=1.0, use_amp=False, num_cascades=12)
    net = S.model.CSModel(cfg)
    net.net_mask.pruned = S.synth.equispaced_pruned(w, 0.25, 0)
    _fill(S, net.net_T, 4235)
    _fill(S, net.net_R, 4236, damp=0.1)
    net.to(DEV).train()
    img_full, img_aux = S.synth.phantom_pair(n, c, h, w, seed=4234)
    out = {}
    try:
        for mode in ("bf16x3", "bf16", "fp16"):
            net.conv_dtype = mode
            with torch.no_grad(), S.ops.conv_precision(mode):
                net.set_input(g(img_full), g(img_aux))
                net.loss_all = 0
                net.forwardT()
                net.forwardR()
            out[mode] = net.img_rec.detach().cpu().clone()
    finally:
        S.ops.set_conv_precision("bf16x3")
    p_bf, p_h = _psnr(out["bf16x3"], out["bf16"]), _psnr(out["bf16x3"], out["fp16"])
    print(f"damped weights, PSNR vs fp32-equivalent: bf16 {p_bf:.1f} dB, fp16 {p_h:.1f} dB")
    assert p_h >= 56.0 and p_h >= p_bf + 10.0, (p_h, p_bf)


@pytest.mark.parametrize("n,cin,cout,h,w,ks", [(2, 72, 36, 40, 40, 3), (1, 18, 36, 160, 160, 3), (2, 64, 96, 32, 48, 1)])
def test_fp16_activations_beyond_the_fp16_range_saturate(S, n, cin, cout, h, w, ks):
    """Forward activations are staged without a scale: magnitudes beyond 65504 saturate to +-65504 (the output stays finite, as in
    the bf16 mode) in the forward convolution and in the weight gradient's activation operand."""
    ops = S.ops
    x = philox("h1.sx", (n, cin, h, w)) * 2
    x[:, :, ::7, ::5] *= 1e5                              # a sprinkle of 1e5-sized activations
    wt = philox("h1.sw", (cout, cin, ks, ks)) * 0.1
    gout = philox("h1.sg", (n, cout, h, w))
    y, _, dw = _run_three(ops, "fp16", x, wt, gout, ks)
    assert torch.isfinite(y).all() and torch.isfinite(dw).all()
    xs = x.clamp(-65504.0, 65504.0)
    q = _ref64(_q16(xs, False), _q16(wt, True), _q16(gout, True), ks)
    assert rel_err(y, q[0]) <= 1e-6 and rel_err(dw, q[2]) <= 1e-6, (rel_err(y, q[0]), rel_err(dw, q[2]))


def _step_model(S, seed_T=71, seed_R=72):
    n, c, h, w = 2, 1, 160, 160
    cfg = S.base.Config(sparsity=0.25, lr=1e-4, shape=w, coils=c, reg="Rec", mask="equispaced", weight_smooth=1000.0,
                        weight_gan=0.0, weight_gan_sim=0.0, weight_sim=1.0, use_amp=False, num_cascades=3)
    net = S.model.CSModel(cfg)
    net.net_mask.pruned = S.synth.equispaced_pruned(w, 0.25, 0)
    _fill(S, net.net_T, seed_T)
    _fill(S, net.net_R, seed_R, damp=0.1)
    net.to(DEV).train()
    batches = [tuple(g(t) for t in S.synth.phantom_pair(n, c, h, w, seed=300 + i)) for i in range(6)]
    return net, batches


def _flat_grads(net):
    return [torch.cat([p.grad.detach().double().flatten().cpu() for p in m.parameters()]) for m in (net.net_R, net.net_T)]


def test_fp16_training_step_gradients(S):
    """One 'Rec' step (forward, hand-written backward, side-stream weight gradients, optimiser) in each mode from the same weights:
    every gradient of the fp16 step is finite and its relative L2 error against the fp32-equivalent step is at most half the bf16
    step's, for each network."""
    grads = {}
    for mode in ("bf16x3", "bf16", "fp16"):
        net, batches = _step_model(S)
        net.conv_dtype = mode
        net.auto_record = False
        net.set_input(*batches[0])
        net.update()
        torch.cuda.synchronize()
        grads[mode] = _flat_grads(net)
    for k, name in enumerate(("R", "T")):
        ref = grads["bf16x3"][k]
        e_h, e_b = rel_err(grads["fp16"][k], ref), rel_err(grads["bf16"][k], ref)
        print(f"net_{name} gradient vs fp32-equivalent: fp16 {e_h:.2e}, bf16 {e_b:.2e} (ratio {e_h / e_b:.3f})")
        assert torch.isfinite(grads["fp16"][k]).all()
        assert e_h <= 0.5 * e_b, (name, e_h, e_b)


def test_fp16_steps_replay_bit_identically(S):
    """The reference's loop ``set_input(batch); update()`` over six batches in the fp16 mode: with auto-recording the third call records
    the step and the rest replay it; parameters and losses are bit-identical to the same loop run eagerly."""
    def loop(auto):
        net, batches = _step_model(S)
        net.conv_dtype = "fp16"
        net.auto_record = auto
        modes = []
        for b in batches:
            net.set_input(*b)
            net.update()
            modes.append(net.step_mode)
        torch.cuda.synchronize()
        return net, modes

    ref, modes_e = loop(False)
    net, modes_a = loop(True)
    assert all(m == "eager" for m in modes_e)
    assert any(m.startswith("replay") for m in modes_a), modes_a
    for m_ref, m_net in ((ref.net_R, net.net_R), (ref.net_T, net.net_T)):
        for (k, a), (_, b) in zip(m_ref.state_dict().items(), m_net.state_dict().items()):
            assert torch.equal(a, b), k
    assert torch.equal(ref.img_rec, net.img_rec)
    assert ref.optim_R.steps_taken() == net.optim_R.steps_taken() == 6
