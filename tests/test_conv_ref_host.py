"""The float64 reference of the single-launch convolution tests (tools/conv_ref.py) against torch on the CPU, so that it cannot be wrong
in the same way as a kernel: with unrounded operands the row gather + matrix product equals torch.nn.functional.conv2d on the NCHW
view of every face, in float64 to 1e-12 relative; the slice-grouped sum equals the plain one; the rounded form equals the unrounded
form of operands that were rounded by tensor.bfloat16() first.  And the inputs cannot hide a leak across a face border: a convolution
that takes the neighbouring face for the padding differs from the reference by a large step at every pixel one of whose taps crosses
a border into real data, and nowhere else.  No GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_ref as CR  # noqa: E402

C, FACES = 32, 3


def _close(got, want):
    assert got.shape == want.shape and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), float((got - want).abs().max() / want.abs().max())


def _operands(kind, side, seed=3):
    g = torch.Generator().manual_seed(seed)
    n, k = (C, 3) if kind == "hca" else (2 * C, 2)
    x = torch.randn(FACES * side * side, C, generator=g, dtype=torch.float64)
    return x, torch.randn(n, C, k, k, generator=g, dtype=torch.float64) / (C * k * k) ** 0.5, torch.randn(n, generator=g, dtype=torch.float64)


def _nchw(x, side):
    return x.reshape(FACES, side, side, -1).permute(0, 3, 1, 2)


def _rows(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


@pytest.mark.parametrize("side", [1, 2, 4, 8])
def test_hca_is_conv2d_pad_1_relu_per_face(side):
    x, w, b = _operands("hca", side)
    _close(CR.evaluate("hca", x, w, b, side, rounded=False), _rows(torch.relu(F.conv2d(_nchw(x, side), w, b, padding=1))))


@pytest.mark.parametrize("side", [2, 4, 8])
def test_down_is_conv2d_2x2_stride_2_per_face(side):
    x, w, b = _operands("down", side)
    _close(CR.evaluate("down", x, w, b, side, rounded=False), _rows(F.conv2d(_nchw(x, side), w, b, stride=2)))


@pytest.mark.parametrize("ks", [2, 4, 8])
def test_the_slice_grouped_sum_is_the_same_sum(ks):
    x, w, b = _operands("hca", 4)
    xb, wb = x.bfloat16().double(), w.bfloat16().double()
    _close(CR.evaluate_sliced(xb, wb, b, 4, ks, dtype=torch.float64), CR.evaluate("hca", xb, wb, b, 4, rounded=False))
    v32 = CR.evaluate_sliced(xb, wb, b, 4, ks)
    assert v32.dtype == torch.float32 and float((v32.double() - CR.evaluate("hca", xb, wb, b, 4)).abs().max()) < 1e-5


@pytest.mark.parametrize("kind,side", [("hca", 1), ("hca", 4), ("down", 4)])
def test_rounding_happens_at_the_operands_and_nowhere_else(kind, side):
    x, w, b = _operands(kind, side)
    x, w = x.float(), w.float()                                   # fp32, as the tests hand them over
    assert torch.equal(CR.round_bf16(w).float(), w.bfloat16().float()) and torch.equal(CR.round_bf16(x).float(), x.bfloat16().float())
    assert torch.equal(CR.evaluate(kind, x, w, b, side), CR.evaluate(kind, x.bfloat16().double(), w.bfloat16().double(), b, side, rounded=False))
    v32 = CR.evaluate(kind, x, w, b, side, dtype=torch.float32)
    assert v32.dtype == torch.float32 and float((v32.double() - CR.evaluate(kind, x, w, b, side)).abs().max()) < 1e-5
    m64, m32 = CR.weight_matrices(w)                              # the prebuilt weight matrices are the same operands
    assert torch.equal(CR.evaluate(kind, x, None, b, side, wm=m64), CR.evaluate(kind, x, w, b, side))
    assert torch.equal(CR.evaluate(kind, x, None, b, side, dtype=torch.float32, wm=m32), v32)


def test_inputs_mark_every_face_and_every_border_pixel():
    for side in (1, 2, 4, 16):
        x = CR.make_input(5, side, 64, seed=1).reshape(5, side * side, 64)
        assert torch.equal(x, x.bfloat16().float()) and float(x.abs().min()) >= 2.0 ** -6 * 0.5      # no zero, border pixels included
        rms = x.pow(2).mean((1, 2)).sqrt()
        assert len({round(float(r), 3) for r in rms}) == 5          # a scale of its own
        sign = torch.sign(x[:, 0])
        assert bool((torch.sign(x) == sign[:, None]).all())         # one sign per (face, channel)
        assert all(not torch.equal(sign[i], sign[j]) for i in range(5) for j in range(i))
    cls = CR.pixel_class(4)
    assert cls.tolist() == [0, 1, 1, 0, 1, 2, 2, 1, 1, 2, 2, 1, 0, 1, 1, 0]
    assert CR.pixel_class(1).tolist() == [0] and CR.pixel_class(2).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("side", [2, 4, 8, 16])
def test_a_conv_that_ignores_face_borders_differs_at_border_pixels_only(side):
    """The leak a kernel with a wrong border test would compute, on the inputs and weights of the GPU test: every pixel with a tap that
    crosses its face's border into real data is off by more than a quarter of the output's rms in some column (rounding noise is five
    orders below), every class of border pixel of every face is hit, and every other pixel is bit for bit the same."""
    faces = 3
    x = CR.make_input(faces, side, 128, seed=2)
    w, b = CR.make_weight("hca", 128)
    ref, leak = CR.evaluate("hca", x, w, b, side), CR.evaluate("hca", x, w, b, side, leak=True)
    crosses = (CR.tap_rows(faces, side, 3, 1, 1) != CR.tap_rows(faces, side, 3, 1, 1, leak=True)).any(1)
    step = (ref - leak).abs().max(1).values
    assert bool((step[crosses] > 0.25 * float(ref.pow(2).mean().sqrt())).all()) and torch.equal(ref[~crosses], leak[~crosses])
    cls = CR.pixel_class(side).repeat(faces)
    face = torch.arange(faces).repeat_interleave(side * side)
    assert not bool(crosses[cls == 2].any())
    for f in range(faces):
        for k in set(cls.tolist()) - {2}:
            assert bool(crosses[(face == f) & (cls == k)].any()), (f, CR.PIXEL_CLASSES[k])
    # the down-conv's taps never leave the face: what can go wrong there is the face a pixel is taken from, which the scales mark
    assert torch.equal(CR.tap_rows(faces, side, 2, 2, 0), CR.tap_rows(faces, side, 2, 2, 0, leak=True))
    wd, bd = CR.make_weight("down", 128)
    d = CR.evaluate("down", x, wd, bd, side)
    swapped = CR.evaluate("down", x.reshape(faces, -1, 128).roll(1, 0).reshape(-1, 128), wd, bd, side)
    assert float((d - swapped).abs().reshape(faces, -1).max(1).values.min()) > 0.25 * float(d.pow(2).mean().sqrt())


def test_staged_table_matches_the_faces_per_workgroup_the_cases_use():
    assert {k: CR.faces_per_workgroup(*k) for k in CR.STAGED} == {(128, 16): 1, (256, 8): 2, (512, 4): 4, (1024, 2): 8, (256, 16): 1, (512, 8): 1,
                                                                   (1024, 4): 4, (2048, 2): 8, (128, 32): 1}


# ---------------------------------------------------------------------------------------------- conv1 -> depthwise 3x3 -> gate -> pool
@pytest.mark.parametrize("side,per_face,stats_np", [(1, False, 1), (2, True, 2), (4, False, 2), (4, True, 1), (8, True, 2)])
def test_dwgate_is_layer_norm_film_conv1_depthwise_conv_and_the_gate(side, per_face, stats_np):
    """Unrounded, in float64: layer_norm over the channels with the row's FiLM gain and bias, conv1 as a 1x1 conv2d, conv2 as a 3x3 pad-1
    conv2d with groups = 2 C on every face, the product of the halves, and its mean per face."""
    Cd, faces = 64, 3
    ops = CR.make_dw_operands(Cd, side, faces, stats_np, per_face=per_face, face0=2, seed=1, exact=True)
    g = torch.Generator().manual_seed(9)
    w1 = torch.randn(2 * Cd, Cd, generator=g, dtype=torch.float64) / 8
    b1, b2 = torch.randn(2 * Cd, generator=g, dtype=torch.float64), torch.randn(2 * Cd, generator=g, dtype=torch.float64)
    w2 = torch.randn(2 * Cd, 1, 3, 3, generator=g, dtype=torch.float64) / 3
    got = CR.evaluate_dw(ops, w1, b1, w2, b2, rounded=False)
    film = ops["film"].double()
    rows = ops["face0"] + torch.arange(ops["M"]) // ops["hw"] if per_face else torch.zeros(ops["M"], dtype=torch.long)
    gain, bias = film[rows, CR.FILM_OFF + Cd:CR.FILM_OFF + 2 * Cd], film[rows, CR.FILM_OFF:CR.FILM_OFF + Cd]
    ln = F.layer_norm(ops["A"], (Cd,), eps=1e-6) * gain + bias
    nchw = lambda t: t.reshape(faces, side, side, -1).permute(0, 3, 1, 2)      # noqa: E731
    t1 = F.conv2d(nchw(ln), w1[:, :, None, None], b1)
    u = F.conv2d(t1, w2, b2, padding=1, groups=2 * Cd)
    gg = u[:, :Cd] * u[:, Cd:]
    _close(got["t1"], _rows(t1))
    _close(got["g"], _rows(gg))
    _close(got["pooled"], gg.mean((2, 3)))


def test_dwgate_operands_are_settled_and_mark_every_face():
    import gemm_ref as G
    ops = CR.make_dw_operands(128, 4, 5, 4, per_face=True, face0=3, seed=2)
    assert torch.equal(ops["A"], ops["A"].bfloat16().float()) and ops["film"].shape[0] == 8
    assert torch.equal(G.a_operand(ops).float(), G.a_operand(ops, torch.float32))       # no element rounds differently in fp32
    rms = ops["A"].reshape(5, -1).pow(2).mean(1).sqrt()
    assert len({round(float(r), 2) for r in rms}) == 5
    sl = CR.dw_slice(ops, 2)
    assert sl["M"] == 32 and sl["A"].shape[0] == 32 and sl["stats_in"].shape[0] == 32
    w1, b1, w2, b2 = CR.make_dw_weights(128)
    full, part = CR.evaluate_dw(ops, w1, b1, w2, b2), CR.evaluate_dw(sl, w1, b1, w2, b2)
    assert torch.equal(full["g"][:32], part["g"]) and torch.equal(full["pooled"][:2], part["pooled"])      # faces are independent
    # a depthwise conv that ignores the face border differs at border pixels: the gate halves of neighbouring faces differ in scale
    t1 = full["t1"]
    idx_leak = CR.tap_rows(5, 4, 3, 1, 1, leak=True)
    tz = torch.cat((t1, torch.zeros(1, t1.shape[1], dtype=t1.dtype)))
    u = b2.double().expand(t1.shape[0], -1).clone()
    for t in range(9):
        u += w2.double().reshape(-1, 9)[:, t] * tz[idx_leak[:, t]]
    leak = u[:, :128] * u[:, 128:]
    crosses = (CR.tap_rows(5, 4, 3, 1, 1) != idx_leak).any(1)
    step = (leak - full["g"]).abs().max(1).values
    assert bool((step[crosses] > 0.25 * float(full["g"].pow(2).mean().sqrt())).all()) and torch.equal(leak[~crosses], full["g"][~crosses])
