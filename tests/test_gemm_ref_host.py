"""The float64 reference of the single-launch GEMM tests (tools/gemm_ref.py) against torch on the CPU, so that it cannot be wrong in
the same way as a kernel: with unrounded operands every family equals the plain composition of torch.nn.functional.linear, layer_norm
with the folded affine, pixel_shuffle on the NHWC -> NCHW view, the gate product and the residual, in float64 to 1e-12 relative; the
partial merge equals var(unbiased=False) of the row; the bf16 rounding equals tensor.bfloat16() bit for bit.  No GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gemm_ref as G  # noqa: E402

N, K, M, HW = 64, 96, 32, 4


def _weights(n=N, k=K):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, k, generator=g, dtype=torch.float64) / k ** 0.5, torch.randn(n, generator=g, dtype=torch.float64)


def _ops(family, **kw):
    W, b = _weights()
    ops = G.make_operands(family, N, K, M, exact=True, seed=3, **kw)
    return dict(ops, W=W, bias=b, N=N, K=K), W, b


def _close(got, want):
    assert got.shape == want.shape and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), float((got - want).abs().max() / want.abs().max())


def _face(ops):
    return torch.arange(ops["M"]) // ops["hw"]


def _ln(ops):
    """layer_norm over the channel axis of the rows the partials describe, then the folded affine of the launch or of the row's face."""
    x, k = ops["A"].double(), ops["A"].shape[1]
    film = ops["film"].double()
    rows = ops["face0"] + _face(ops) if ops["per_face"] else torch.zeros(ops["M"], dtype=torch.long)
    gain, bias = film[rows, ops["gain_off"]:ops["gain_off"] + k], film[rows, ops["bias_off"]:ops["bias_off"] + k]
    if not ops["per_face"]:
        return F.layer_norm(x, (k,), gain[0], bias[0], eps=1e-6)
    return F.layer_norm(x, (k,), eps=1e-6) * gain + bias


@pytest.mark.parametrize("act", [0, 1, 2])
def test_f32_biasf32(act):
    ops, W, b = _ops("f32_biasf32", act=act)
    y = F.linear(ops["A"].double() * ops["a_scale"], W, b)
    _close(G.evaluate(ops, rounded=False)["v"], [y, torch.relu(y), torch.sigmoid(y)][act])


def test_bf16_biasf32_and_biasbf16():
    ops, W, b = _ops("bf16_biasf32")
    _close(G.evaluate(ops, rounded=False)["v"], F.linear(ops["A"].double(), W, b))
    ops, W, b = _ops("bf16_biasbf16", act=1)
    _close(G.evaluate(ops, rounded=False)["v"], torch.relu(F.linear(ops["A"].double(), W, b) + ops["resid"].double()))


@pytest.mark.parametrize("family", ["bf16_resid", "bf16s_resid"])
def test_resid_and_its_gated_output(family):
    ops, W, b = _ops(family, hw=HW, gated=True)
    a = ops["A"].double() * (ops["rowscale"].double()[_face(ops)] if family == "bf16s_resid" else 1.0)
    v = ops["resid"].double() + ops["rscale"].double() * F.linear(a, W, b)
    got = G.evaluate(ops, rounded=False)
    _close(got["v"], v)
    _close(got["g"], (v + ops["add_src"].double()) * (1.0 + ops["gate_c"].double()[_face(ops)] + ops["gate_s"].double()[:, None]))


@pytest.mark.parametrize("per_face", [False, True])
@pytest.mark.parametrize("stats_np", [1, K // 32])
def test_layernorm_families(per_face, stats_np):
    ops, W, b = _ops("ln_biasf32", hw=HW, per_face=per_face, face0=3 if per_face else 0, stats_np=stats_np)
    assert float(ops["ratio"].max()) >= 30.0                      # the offset rows are there
    _close(G.evaluate(ops, rounded=False)["v"], F.linear(_ln(ops), W, b))
    ops, W, b = _ops("ln_gate", hw=HW, per_face=per_face, face0=3 if per_face else 0, stats_np=stats_np)
    h = F.linear(_ln(ops), W, b)
    _close(G.evaluate(ops, rounded=False)["v"], h[:, :N // 2] * h[:, N // 2:])


def test_per_face_rows_are_distinct_and_start_at_face0():
    ops, _, _ = _ops("ln_biasf32", hw=HW, per_face=True, face0=3)
    assert ops["film"].shape[0] == 3 + M // HW and len({tuple(r.tolist()) for r in ops["film"]}) == ops["film"].shape[0]
    a = G.a_operand(ops, rounded=False)
    ops2 = dict(ops, face0=2)
    assert not torch.equal(a, G.a_operand(ops2, rounded=False))


@pytest.mark.parametrize("family", ["f32_pixshuf", "bf16_pixshuf"])
@pytest.mark.parametrize("r", [1, 2])
def test_pixel_shuffle(family, r):
    win = 2
    ops, W, _ = _ops(family, shuffle_r=r, win=win)
    y = F.linear(ops["A"].double() * ops.get("a_scale", 1.0), W)
    if r == 2:
        nchw = y.reshape(M // (win * win), win, win, N).permute(0, 3, 1, 2)
        y = F.pixel_shuffle(nchw, 2).permute(0, 2, 3, 1).reshape(4 * M, N // 4)
    _close(G.evaluate(ops, rounded=False)["v"], y + ops["resid"].double())


@pytest.mark.parametrize("stats_np", [1, 3, K // 32])
def test_partial_merge_is_the_biased_variance_of_the_row(stats_np):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g, dtype=torch.float64) * 3 + 50 * torch.randn(M, 1, generator=g, dtype=torch.float64)
    t = x.reshape(M, stats_np, K // stats_np)
    mean = t.mean(-1)
    stats = torch.stack((mean, (t - mean[..., None]).pow(2).sum(-1)), -1)
    m, rstd = G.merge_partials(stats, K // stats_np)
    assert float((m - x.mean(1)).abs().max()) <= 1e-12 * float(x.mean(1).abs().max())
    var = 1.0 / rstd ** 2 - G.LN_EPS
    assert float((var - x.var(1, unbiased=False)).abs().max()) <= 1e-12 * float(x.var(1, unbiased=False).max())
    ts = G.tile_stats(x)
    assert torch.allclose(ts[..., 0], x.reshape(M, -1, 32).mean(-1), rtol=1e-13, atol=0)
    assert torch.allclose(ts[..., 1], x.reshape(M, -1, 32).var(-1, unbiased=False) * 32, rtol=1e-12, atol=0)


def _bits(t):
    return t.float().view(torch.int32)


def test_round_bf16_is_tensor_bfloat16_bit_for_bit():
    g = torch.Generator().manual_seed(17)
    x = torch.randn(1_000_000, generator=g) * torch.exp2(torch.randint(-30, 30, (1_000_000,), generator=g).float())
    grid = x[:200_000].bfloat16().float()
    half = (G.bf16_ulp(grid) / 2).float()
    ties = torch.cat((grid + half, grid - half))                 # exact midpoints (fp32 holds them): round to even
    assert bool(((ties.view(torch.int32) & 0xFFFF) == 0x8000).sum() > 300_000)
    tiny = torch.cat((torch.randn(50_000, generator=g) * 2.0 ** -130, torch.arange(-300, 300).float() * 2.0 ** -134,
                      torch.tensor([0.0, -0.0, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, G.BF16_MAX, -G.BF16_MAX,
                                    3.4e38, -3.4e38, float("inf"), -float("inf")])))
    for batch in (x, ties, tiny):
        assert torch.equal(_bits(G.round_bf16(batch)), _bits(batch.bfloat16())), "float32 input"
        assert torch.equal(_bits(G.round_bf16(batch.double())), _bits(batch.bfloat16())), "float64 input"
    assert bool(torch.isnan(G.round_bf16(torch.tensor([float("nan")]))).all())
    assert float(G.tie_distance(torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64))) == 0.0
    assert float(G.tie_distance(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -8


def test_rounded_reference_rounds_at_the_kernels_points_only():
    """float64 with rounding on: the weight and the transformed A operand are bf16 values, the accumulation and the epilogue are not
    rounded; the fp32 evaluation of the same operands differs from it by fp32 noise only."""
    W, b = _weights()
    ops = dict(G.make_operands("ln_gate", N, K, M, hw=HW, per_face=True, face0=3, stats_np=3, seed=3), W=W.float(), bias=b.float(), N=N, K=K)
    a = G.a_operand(ops)
    assert torch.equal(a, G.round_bf16(a)) and not torch.equal(a, G.a_operand(ops, rounded=False))
    assert torch.equal(a.float(), G.a_operand(ops, torch.float32))      # settle_ln: both evaluations round A alike
    v64, v32 = G.evaluate(ops)["v"], G.evaluate(ops, torch.float32)["v"]
    assert v32.dtype == torch.float32 and 0 < float((v32.double() - v64).abs().max()) < 1e-5
    want = F.linear(a, G.round_bf16(W), b.float().double())
    _close(v64, want[:, :N // 2] * want[:, N // 2:])


def test_settle_ln_moves_few_elements_and_reports_what_it_cannot_settle():
    ops = G.make_operands("ln_biasf32", N, 256, 64, stats_np=8, seed=9)
    assert 0 < ops["moved"] < 0.2 * 64 * 256
    assert torch.equal(ops["A"], ops["A"].bfloat16().float())
    film = torch.zeros_like(ops["film"])
    film[:, ops["bias_off"]:ops["bias_off"] + 256] = 1.0 + 2.0 ** -8      # gain 0, bias on a tie: no move of x takes the value off it
    bad = dict(ops, film=film)
    with pytest.raises(ValueError):
        G.settle_ln(bad, max_iter=4)
