"""VAE boundary (hd_vae_encode / hd_vae_decode), launch by launch: every launch of both programs against the CPU oracle on the
launch's own inputs (tools/vae_forced.py), at the bounds of the denoiser's teacher-forced scan -- 3e-4 rel-L2 for fp32 outputs,
3e-3 for bf16-stored outputs, bit-exact for pure data movement -- on the plain synthetic weights and on a `stress` set that
makes the softmax sharp (logits past exp's fp32 range), GroupNorm's input far from centred and the posterior's logvar reach both
ends of its clamp.  test_vae_boundary_against_oracle (test_gpu_parity.py) keeps the end-to-end view.  Figures: profiles/r11_vae_ops.txt."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def weight_sets():
    import vae_forced
    from hifidiff_amd import synth
    torch.set_grad_enabled(False)
    P = synth.vae_state_dict()
    return {"plain": P, "stress": vae_forced.stress_state_dict(P)}


@pytest.fixture(scope="module")
def vaes(gpu, weight_sets):
    """One AutoencoderKL per weight set, made when first asked for."""
    from hifidiff_amd.vae import AutoencoderKL
    made = {}

    def get(which):
        if which not in made:
            v = AutoencoderKL()
            v.load_state_dict(weight_sets[which])
            made[which] = v.to("cuda:0")
        return made[which]
    return get


def _faces(B, R):
    from hifidiff_amd import synth
    return T(np.stack([synth.rand(f"cr_face_vae/{f}", (3, R, R)) for f in range(B)]))


def _latents(B, Lr):
    from hifidiff_amd import synth
    return T(np.stack([np.float32(0.8) * synth.randn(f"vae_z/{f}", (4, Lr, Lr)) for f in range(B)]))


def _noise(B, Lr):
    from hifidiff_amd import synth
    return T(np.stack([synth.randn(f"vae_noise/{f}", (4, Lr, Lr)) for f in range(B)]))


@pytest.fixture(scope="module")
def scans(vaes, weight_sets):
    """(weights, side, B) -> (report, worst per launch kind, statistics of the inputs read back) of the full scan at 64 px / latent 8: run once,
    shared by the tests that look at it."""
    import vae_forced
    done = {}

    def get(weights, side, B):
        key = (weights, side, B)
        if key not in done:
            report, info = [], {}
            if side == "encode":
                worst = vae_forced.encode_scan(vaes(weights), weight_sets[weights], _faces(B, 64), 64, report, noise=_noise(B, 8), info=info)
            else:
                worst = vae_forced.decode_scan(vaes(weights), weight_sets[weights], _latents(B, 8), report, info=info)
            print(f"---- {weights} {side} batch {B}\n" + "\n".join(report) + f"\nworst {worst}\ninputs {info}")
            done[key] = (report, worst, info)
        return done[key]
    return get


def _require_sharp(st, what):
    """The stress weights must have made this attention input sharp: an input error otherwise, not a kernel error."""
    if not (st["median_maxp"] >= 0.5 and st["logit_absmax"] > 88.0 and (st["T"] <= 64 or st["argmax_past_tile0"] >= 0.25)):
        pytest.fail(f"input error: the stress weights do not make {what} sharp: {st}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("side", ["encode", "decode"])
@pytest.mark.parametrize("weights", ["plain", "stress"])
def test_every_vae_launch_against_oracle_on_its_own_inputs(scans, weights, side, B):
    """Full scan of encode (64 -> 64 px, posterior sample with given noise, then the moments form of the last launch) and decode
    (latent 8) at batch 1 and 3 (M = 64 B rows at the deepest level, odd B), plain and stress weights: every launch has a rule and
    is within its bound.  The stress set must have produced what it is for, measured on the values read back: |group mean| /
    group std >= 30 at the first norm1 after conv_in, median max-probability >= 0.5 and logit abs-max > 88 at the attention, and
    (encode) >= 1 % of logvar below -30 and >= 1 % above 20.
    Measured (profiles/r11_vae_ops.txt), worst rel-L2 over the eight scans: GroupNorm 6.5e-4 (stress; 1.1e-4 plain), softmax_qk_v
    9.4e-5, the 3x3 convs 1.6e-6, to_out 1.1e-6, every other GEMM launch <= 3.3e-7, quant_conv + sample 9.5e-8, post_quant_conv 0; the
    data-movement launches differ in 0 elements.  Read back on the stress set: |group mean| / group std 42.7-46.3, median
    max-probability 0.87-0.9997 with logits up to 152, 32 % of logvar below -30 and 39 % above 20."""
    import vae_forced
    report, worst, info = scans(weights, side, B)
    first_norm = ("encoder.down_blocks.0.resnets.0.norm1" if side == "encode" else "decoder.mid_block.resnets.0.norm1")
    attn = ("encoder" if side == "encode" else "decoder") + ".mid_block.attentions.0.softmax_qk_v"
    if weights == "stress":
        if not info["gn_ratio"][first_norm] >= 30.0:
            pytest.fail(f"input error: |group mean| / group std at {first_norm} is {info['gn_ratio'][first_norm]:.1f} < 30")
        _require_sharp(info["attn"][attn], attn)
        if side == "encode" and not (info["logvar"][0] >= 0.01 and info["logvar"][1] >= 0.01):
            pytest.fail(f"input error: logvar does not reach both ends of the clamp: {info['logvar']}")
    assert worst["launches"] == (vae_forced.ENC_OPS if side == "encode" else vae_forced.DEC_OPS)      # a new launch cannot go unchecked
    flagged = [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    assert not flagged, "\n".join(flagged)
    exact = ("encoder.input", "nearest", "decoder.output", "post_quant_conv.pad")
    for kind, w in worst.items():
        if kind in exact:
            assert w == 0, (kind, w)
        elif kind != "launches":
            assert w <= (vae_forced.BF16_BOUND if kind in ("groupnorm", "softmax_qk_v", "post_quant_conv") else vae_forced.FP32_BOUND), (kind, w)
    kinds = {"encode": {"encoder.input", "conv_in", "groupnorm", "conv3x3", "conv_shortcut", "downsample", "linear", "softmax_qk_v", "to_out", "conv_out", "quant_conv.sample"},
             "decode": {"post_quant_conv", "post_quant_conv.pad", "conv_in", "groupnorm", "conv3x3", "conv_shortcut", "linear", "softmax_qk_v", "to_out", "nearest", "upsample_conv",
                        "conv_out", "decoder.output"}}[side]
    assert set(worst) - {"launches"} == kinds


def test_scan_holds_the_border_and_shape_edges(scans):
    """The launches only the VAE gives the shared GEMM family are in the scan by name, and within their bounds: the stride-2
    downsampler convs (zeros read past the right and bottom edge) over the whole map and over the last output row and column
    separately, encoder.conv_out (N = 8), decoder.conv_out (N = 3), the conv_in's (cin 3 / 4 padded to 8) and the conv_shortcut
    1x1s on the fp32 loader."""
    for weights in ("plain", "stress"):
        enc, dec = scans(weights, "encode", 3)[0], scans(weights, "decode", 3)[0]
        for i in range(3):
            name = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            for what in ("X", "last row", "last col"):
                got = [ln for ln in enc if f" {name} " in ln and f" {what:8s} rel " in ln]
                assert len(got) == 1 and "<<<<<<" not in got[0], (name, what, got)
        wanted = [(enc, "encoder.conv_out"), (dec, "decoder.conv_out"), (enc, "encoder.conv_in"), (dec, "decoder.conv_in")]
        wanted += [(enc, f"encoder.down_blocks.{i}.resnets.0.conv_shortcut") for i in (1, 2)]
        wanted += [(dec, f"decoder.up_blocks.{i}.resnets.0.conv_shortcut") for i in (2, 3)]
        for report, name in wanted:
            got = [ln for ln in report if f" {name} " in ln and " rel " in ln]
            assert len(got) == 1 and "<<<<<<" not in got[0], (name, got)
        assert sum(".conv_shortcut " in ln for ln in enc + dec) == 4


ATTN_CASES = {"encode 128 px, batch 2 (T = 256)": ("encode", 128, 2), "encode 256 px, batch 1 (T = 1024)": ("encode", 256, 1), "decode latent 16, batch 2 (T = 256)": ("decode", 16, 2)}


@pytest.mark.parametrize("case", list(ATTN_CASES))
@pytest.mark.parametrize("weights", ["stress", "plain"])
def test_attention_over_several_key_tiles(vaes, weights, case):
    """64 px has T = 64, exactly one AT_K tile of vae_attention_kernel; the rescale of the running sum and of the accumulators
    between key tiles needs more.  The programs run up to `...softmax_qk_v` at T = 256 (4 tiles) and T = 1024 (16 tiles); Q, K, V
    are the to_q / to_k / to_v outputs, the reference is softmax(Q K^T / sqrt(512)) V in float64 rounded to bf16, bound 3e-3.
    With the stress weights the input must be sharp (median max-probability >= 0.5, logit abs-max > 88) with the arg-max key
    outside the first 64-key tile for at least a quarter of the queries, so that the running max moves after the first tile.
    Measured rel-L2, stress / plain: encode T = 256 4.4e-5 / 3.1e-5, encode T = 1024 4.1e-5 / 5.2e-5, decode T = 256 7.1e-5 / 3.0e-5;
    stress inputs: median max-probability 0.56 / 0.57 / 0.99, logit abs-max 137 / 132 / 148, arg-max past the first tile for
    59 % / 100 % / 83 % of the queries."""
    import vae_forced
    side, res, B = ATTN_CASES[case]
    vae = vaes(weights)
    rep = []
    if side == "encode":
        xd = _faces(B, res).cuda()
        rel, st = vae_forced.attention_prefix(vae, 0, lambda: vae._encode(xd, res, False, True, None, 0), B, rep)
    else:
        zd = _latents(B, res).cuda()
        rel, st = vae_forced.attention_prefix(vae, 1, lambda: vae.decode_scaled(zd), B, rep)
    print(f"{weights}, {case}: rel {rel:.3e}; {st}")
    assert st["T"] == {128: 256, 256: 1024, 16: 256}[res]
    if weights == "stress":
        _require_sharp(st, case)
    assert rel <= vae_forced.BF16_BOUND, rep


BICUBIC_PAIRS = [(8, 64), (37, 64), (100, 128), (128, 64), (200, 128), (128, 192), (128, 256)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pair", BICUBIC_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_bicubic_alone(vaes, pair, B):
    """bicubic_resize_kernel on its own (limit 1, launch 0) at non-integer, down- and up-scaling ratios, against
    F.interpolate(mode="bicubic", align_corners=False) in float64, on uniform images and on an image of +-1e3 steps (overshoot, border
    taps).  Allowed max-abs error: 4 x the error torch's own fp32 CPU bicubic has against that float64 result on the same input
    (tap order and FMA contraction differ, nothing else should).  Measured (kernel, torch fp32), uniform images: 1.5e-7 .. 2.8e-7
    against 1.6e-7 .. 3.3e-7, and 8.8e-6 against 8.7e-6 at 128 -> 192 (the only ratio whose scale is not exact in fp32); +-1e3
    steps: 1.6e-4 .. 3.0e-4 against 1.8e-4 .. 8.0e-4, 2.4e-2 against 2.4e-2 at 128 -> 192, and 0 against 0 at 128 -> 64 and
    128 -> 256 (exact weights).  The worst ratio kernel / torch is 1.33 (8 -> 64, batch 3, uniform)."""
    import vae_forced
    from hifidiff_amd import synth
    r, R = pair
    vae = vaes("plain")
    x = T(np.stack([synth.rand(f"bicubic/{f}", (3, r, r)) for f in range(B)]))
    steps = torch.where(T(np.stack([synth.rand(f"bicubic_steps/{f}", (3, r, r)) for f in range(B)])) < 0.5, -1e3, 1e3).to(torch.float32)
    for what, img in (("uniform", x), ("steps", steps)):
        name, got = vae_forced.first_op(vae, img, R)
        assert name == "bicubic" and got.numel() == B * 3 * R * R
        err, err32 = vae_forced.bicubic_errors(got, img, R)
        print(f"bicubic {r} -> {R}, batch {B}, {what}: kernel {err:.3e}, torch fp32 {err32:.3e}")
        assert err <= 4.0 * err32, (what, err, err32)


@pytest.mark.parametrize("vae_range", [False, True])
def test_encoder_input_is_bit_exact(vaes, vae_range):
    """nchw_to_nhwc8_bf16_kernel: NCHW fp32 -> channels-last bf16 x 8 (channels 3..7 zero) is data movement plus one rounding, so
    it must equal RNE-bf16 of the same fp32 values in the right places bit for bit -- with and without to_vae_range
    (clamp(0, 1) * 2 - 1), on values outside [0, 1]."""
    import vae_forced
    from hifidiff_amd import synth
    B, R = 3, 64
    x = T(np.stack([synth.rand(f"vae_input/{f}", (3, R, R)) for f in range(B)])) * 3.0 - 1.0
    assert float(x.min()) < -0.5 and float(x.max()) > 1.5
    name, got = vae_forced.first_op(vaes("plain"), x, R, vae_range=vae_range)
    assert name == "encoder.input"
    v = x.clamp(0, 1) * 2.0 - 1.0 if vae_range else x
    want = torch.zeros(B, R * R, 8)
    want[:, :, :3] = v.to(torch.bfloat16).to(torch.float32).reshape(B, 3, -1).permute(0, 2, 1)
    assert torch.equal(got.view(torch.int32), want.reshape(-1).view(torch.int32))
