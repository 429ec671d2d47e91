"""The face-geometry kernels one launch at a time against float64, at the face counts the network scans do not sit on: the HCA 3x3
conv staged in LDS (hd_conv.hpp, all nine ConvCfg of add_hca's table), the same conv as a patch gather and with the centre tap only
(LdConv in hd_gemm.hpp), the 2x2 stride-2 down-conv, and conv1 -> depthwise 3x3 -> SimpleGate -> pool fused into conv1's epilogue
(EpDwGate1, every branch of dispatch_dwgate), by strips (hd_strip.hpp) and unfused (dwconv_gate_pool + pool_finish).  Every launch goes
through `hd_debug_conv`, i.e. through the library's own add_hca / add_down / add_conv1_dwgate (the function the block builder calls):
the kernel is chosen by the library from (C, side, M, the partials' form), never forced, and what ran is read from the launch note.
Operands, reference and runner: tools/conv_ref.py (held against torch without a GPU by tests/test_conv_ref_host.py, which also shows
that a read across a face border cannot hide in these inputs).

Per launch, the rules of tests/test_gemm_edges.py: fp32 `out` max-abs against float64 <= forced.F64_MARGIN x the max-abs error of the
same evaluation in torch fp32 on the CPU and rel-L2 <= forced.FP32_BOUND; out16 bit for bit the bf16 rounding of the stored `out` and
within ulp / 2 + F64_MARGIN x e32 of float64; stats_out under forced.Check's statistics rule at STAT_BOUND; 64 guard rows behind every
output still hold the NaN pattern they were filled with; a second launch gives the same bits.  The input has 64 rows of the same
pattern behind M, so a read of a face that does not exist shows as NaN; it is read back unchanged.
Per face, added here: rel-L2 of every single face <= FP32_BOUND, and the report names the worst face and the worst class of pixel
(corner, edge, interior), so that a leak across a border names itself.

Face counts: with fpw whole faces per workgroup {1, 2, 3, fpw - 1, fpw, fpw + 1, 2 fpw + 1}.  Figures: profiles/r26_conv_edges.txt."""
import os
import sys
import time

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

HD_ERR_INVALID = -1
STAGED = [(128, 16), (128, 32), (256, 8), (256, 16), (512, 4), (512, 8), (1024, 2), (1024, 4), (2048, 2)]      # by C: one weight conversion per C
GATHER = [(512, 16, (1, 3)), (1024, 8, (1, 3)), (2048, 4, (1, 3)), (2048, 1, (1, 3, 33))]                       # (2048, 1): centre tap only
DOWN = [(128, 16, (1, 3, 9)), (256, 8, (1, 3, 9)), (512, 4, (1, 3, 9)), (1024, 2, (1, 3, 9)), (128, 32, (16,))]


def face_counts(fpw):
    return sorted({1, 2, 3, fpw - 1, fpw, fpw + 1, 2 * fpw + 1} - {0})


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


class State:
    def __init__(self, CR):
        self.CR, self.R = CR, CR.DwRunner()
        self.worst = {}                                          # kernel note -> [fp32 ratio, (err, e32), bf16 excess, launches, sliced ratio]
        self.faces = {}                                          # kernel note -> (worst per-face rel-L2, face, worst pixel class)
        self.stat_worst = 0.0
        self.t0 = time.time()
        self._wm = (None, None)
        self.dw_worst = {}                                       # depthwise kernel note -> [G excess, pooled ratio, T1 ratio, launches, worst face, pixels]
        self.dw_seen = set()                                     # (case id, family, rows, wide form, per_face, stats_np == 1, ragged)

    def matrices(self, kind, C):
        """(float64, fp32) weight matrices of (kind, C); the last pair is kept (302 + 151 MB at C = 2048)."""
        if self._wm[0] != (kind, C):
            self._wm = (None, None)
            self._wm = ((kind, C), self.CR.weight_matrices(self.R.weight(kind, C)[0]))
        return self._wm[1]


@pytest.fixture(scope="module")
def S(gpu):
    import conv_ref as CR
    s = State(CR)
    yield s
    s.R.close()


# ---------------------------------------------------------------------------------------------- the checks of one launch
def _bf16_rule(got, v64, e32, margin):
    """max over the elements of (|got - v64| - ulp / 2) / (margin * e32) (<= 1 passes; e32 = 0: any excess is inf)."""
    import gemm_ref as G
    ulp = G.bf16_ulp(v64.abs() + margin * e32)
    excess = (got.double() - v64).abs() - ulp / 2
    if not bool((excess == excess).all()):
        return float("inf")
    worst = float(excess.max())
    return 0.0 if worst <= 0 else (worst / (margin * e32) if e32 > 0 else float("inf"))


def reference(S, kind, C, side, faces, seed=0):
    """(x, float64, torch fp32[, fp32 in the staged kernel's slice grouping]) of a case at its largest face count."""
    CR = S.CR
    x = CR.make_input(faces, side, C, seed)
    _, b = S.R.weight(kind, C)
    m64, m32 = S.matrices(kind, C)
    ref = [x, CR.evaluate(kind, x, None, b, side, wm=m64), CR.evaluate(kind, x, None, b, side, dtype=torch.float32, wm=m32)]
    if kind == "hca" and (C, side) in CR.STAGED:
        ref.append(CR.evaluate_sliced(x, None, b, side, CR.STAGED[(C, side)][1], wm=m32))
    return ref


def check_launch(S, kind, C, side, faces, ref, label):
    """Launches the first `faces` faces of the case twice and applies every assertion of the module docstring.  Returns the note."""
    import forced
    CR, R = S.CR, S.R
    hw = side * side
    M = faces * hw
    x = ref[0][:M]
    rc, note, got = R.launch(kind, x, C, side)
    assert rc == 0, (label, faces, R.error())
    rc2, _, again = R.launch(kind, x, C, side)
    assert rc2 == 0, (label, faces, R.error())
    rows = M if kind == "hca" else M // 4
    v64, v32 = ref[1][:rows], ref[2][:rows].double()
    e32 = float((v32 - v64).abs().max())
    where = f"{label} faces {faces} [{CR.note_key(kind, note)}]"
    xin = got.pop("_x")
    assert CR.same_bits(xin[:M], x.bfloat16()) and CR.untouched(xin[M:]), f"{where}: the input changed"
    again.pop("_x")
    for k, t in got.items():
        assert CR.untouched(t[rows:]), f"{where}: {k} written past row {rows}"
        assert CR.same_bits(t, again[k]), f"{where}: {k} differs between two launches"
    body = got["out"][:rows]
    d = (body.double() - v64).abs()
    d = torch.where(d == d, d, torch.full_like(d, float("inf")))
    err, rel = float(d.max()), float(d.norm() / v64.norm().clamp_min(1e-30))
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
    pf = d.reshape(faces, -1).norm(dim=1) / v64.reshape(faces, -1).norm(dim=1).clamp_min(1e-30)
    cls = CR.pixel_class(side if kind == "hca" else side // 2).repeat(faces)
    per_class = {CR.PIXEL_CLASSES[k]: float(d[cls == k].max()) for k in sorted(set(cls.tolist()))}
    wface, wcls = int(pf.argmax()), max(per_class, key=per_class.get)
    sliced = float("nan")
    if len(ref) > 3:
        e32s = float((ref[3][:rows].double() - v64).abs().max())
        sliced = err / e32s if e32s > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{where}: maxabs {err:.3e} torch fp32 {e32:.3e} ratio {ratio:.2f} (slice-grouped fp32: {sliced:.2f}) rel {rel:.3e}; worst face {wface} "
          f"rel {float(pf.max()):.3e}; worst pixels {wcls} " + " ".join(f"{k} {v:.3e}" for k, v in per_class.items()))
    assert err <= forced.F64_MARGIN * e32 and rel <= forced.FP32_BOUND, \
        f"{where}: maxabs {err:.3e} vs torch fp32 {e32:.3e}, rel {rel:.3e}; worst face {wface}, worst pixels {wcls} {per_class}"
    assert float(pf.max()) <= forced.FP32_BOUND, f"{where}: face {wface} rel {float(pf.max()):.3e}; worst pixels {wcls} {per_class}"
    assert CR.same_bits(got["out16"][:rows], body.bfloat16()), f"{where}: out16 is not the bf16 rounding of the stored out"
    excess = _bf16_rule(got["out16"][:rows], v64, e32, forced.F64_MARGIN)
    assert excess <= 1.0, f"{where}: out16 beyond ulp / 2 + {forced.F64_MARGIN} x the fp32 error by a factor {excess:.3g}"
    if "stats_out" in got:
        rep = []
        me, re_, _ = forced.Check(rep).stats(0, label, "stats_out", got["stats_out"][:rows].reshape(-1), body, body.shape[1] // 32, 32)
        S.stat_worst = max(S.stat_worst, me, re_)
        assert me <= forced.STAT_BOUND and re_ <= forced.STAT_BOUND, f"{where}: {rep[-1]}"
    key = CR.note_key(kind, note)
    w = S.worst.setdefault(key, [0.0, (0.0, 0.0), 0.0, 0, 0.0])
    if ratio >= w[0]:
        w[0], w[1] = ratio, (err, e32)
    w[2], w[3], w[4] = max(w[2], excess), w[3] + 1, max(w[4], sliced if sliced == sliced else 0.0)
    if float(pf.max()) >= S.faces.get(key, (0.0,))[0]:
        S.faces[key] = (float(pf.max()), wface, wcls)
    return note


# ---------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("C,side", STAGED, ids=[f"C{c}-side{s}" for c, s in STAGED])
def test_staged_hca_conv_at_face_counts_that_do_not_fill_a_workgroup(S, C, side):
    """All nine (C, side) pairs of add_hca's table at {1, 2, 3, fpw - 1, fpw, fpw + 1, 2 fpw + 1} faces: the workgroup whose faces past M
    are clamped and zeroed, borders between faces that lie next to each other in LDS, the strip form and, for C >= 1024, the XCD tile
    remap with gridDim.x = 2 and a ragged second row group (asserted from the note).  K = 9 C up to 18432, summed in KS slices.
    Measured (profiles/r26_conv_edges.txt), worst max-abs error as a multiple of torch's fp32 error (bound 4): 2.34 (C 256 side 16), 1.75
    (C 128 side 16), 1.55 (the strip form), 1.51 at K = 18432 (C 2048 side 2), <= 1.01 with the remap and a ragged group; as a multiple
    of an fp32 evaluation in the kernel's own slice grouping <= 2.89 (printed, not a bound: no case needed it); worst face rel-L2
    1.8e-7; out16 beyond half an ulp by at most 0.15 of the allowed 4 x e32."""
    CR = S.CR
    fpw = CR.faces_per_workgroup(C, side)
    counts = face_counts(fpw)
    ref = reference(S, "hca", C, side, max(counts))
    bm, ks, nt, strip = CR.STAGED[(C, side)]
    for faces in counts:
        note = check_launch(S, "hca", C, side, faces, ref, f"hca C {C} side {side}")
        have = (note["form"], note["C"], note["side"], note["bm"], note["ks"], note["nt"], note["strip"], note["faces_per_wg"])
        if have != (1, C, side, bm, ks, nt, strip, fpw):
            pytest.fail(f"input error: hca C {C} side {side} ran {have}, not the staged ConvCfg {(1, C, side, bm, ks, nt, strip, fpw)}")
        assert note["grid_x"] == -(-faces * side * side // bm) and note["grid_y"] == C // (32 * nt), note
        if C >= 1024:
            assert note["remap"] == (1 if note["grid_x"] > 1 else 0), note
            if faces == fpw + 1:
                assert note["remap"] == 1 and note["grid_x"] == 2 and note["grid_y"] % 8 == 0, note
        else:
            assert note["remap"] == 0, note


@pytest.mark.parametrize("C,side,counts", GATHER, ids=[f"C{c}-side{s}" for c, s, _ in GATHER])
def test_hca_conv_as_a_patch_gather_and_with_the_centre_tap_only(S, C, side, counts):
    """(C, side) pairs outside add_hca's table run the same conv through LdConv: (512, 16), (1024, 8), (2048, 4) at 1 and 3 faces, and 1 x 1
    faces at C = 2048 (centre tap only, K = C) at 1, 3 and 33 faces.  Measured (profiles/r26_conv_edges.txt): worst ratio 1.10 (gather),
    0.87 (centre only); worst face rel-L2 2.7e-7; out16 excess <= 0.10."""
    ref = reference(S, "hca", C, side, max(counts))
    for faces in counts:
        note = check_launch(S, "hca", C, side, faces, ref, f"hca C {C} side {side}")
        if note["form"] != 2 or note["centre_only"] != (1 if side == 1 else 0) or note["gemm"]["family"] == 0:
            pytest.fail(f"input error: hca C {C} side {side} did not run the patch gather: {note}")


@pytest.mark.parametrize("C,side,counts", DOWN, ids=[f"C{c}-side{s}" for c, s, _ in DOWN])
def test_down_conv_with_copy_and_statistics(S, C, side, counts):
    """Source pairs (128, 16), (256, 8), (512, 4), (1024, 2) at 1, 3 and 9 faces, and (128, 32) at 16 faces, where dst.M = 4096 and add_down
    asks for 32-row tiles (asserted from the note); out, out16 and stats_out per 32-column tile.  Measured (profiles/r26_conv_edges.txt):
    worst ratio 1.02, worst face rel-L2 1.4e-7, out16 excess <= 0.06, stats_out <= 1.03e-7 (bound 3e-4)."""
    ref = reference(S, "down", C, side, max(counts))
    for faces in counts:
        note = check_launch(S, "down", C, side, faces, ref, f"down C {C} side {side}")
        if note["form"] != 2 or note["gemm"]["family"] == 0:
            pytest.fail(f"input error: down C {C} side {side} did not run the patch gather: {note}")
        big = faces * side * side // 4 >= 4096
        assert note["hint"] == (3 if big else -1) and (not big or (note["mode"] == 3 and note["gemm"]["rows"] == 32)), note


# ---------------------------------------------------------------------------------------------- conv1 -> depthwise 3x3 -> gate -> pool
# (id, C, side, face counts, ((per-face FiLM, stats_np), ...), (kernel family, rows per workgroup, wide form)): each branch of dispatch_dwgate
# at the smallest M at which the library's rules (hd_dispatch.hpp, deep_shape_ok, wide_shape_ok as they stand) give it, and where the
# shape rule allows a ragged last tile, one face short of a full one
FUSED = [
    ("EpDwGate1", 2048, 1, (1, 3, 33), ((False, 1), (False, 64), (True, 64)), (3, (16, 32), 0)),
    ("skinny<1,1> hw 16", 512, 4, (1, 2, 3, 5), ((False, 1), (False, 16), (True, 16)), (3, (16, 32), 0)),
    ("skinny<1,1> hw 4", 1024, 2, (7, 8, 9), ((False, 32), (True, 1)), (3, (16, 32), 0)),
    ("skinny<1,2> shared", 256, 4, (256,), ((False, 8),), (3, (64,), 0)),
    ("skinny<1,2> per-face", 2048, 2, (64,), ((True, 64),), (3, (64,), 0)),
    ("skinny<2,1>", 256, 8, (1, 2, 3), ((False, 8), (True, 1)), (3, (64,), 0)),
    ("skinny<8,1> hw 64", 256, 8, (128,), ((False, 8),), (3, (256,), 0)),
    ("skinny<8,1> hw 256", 128, 16, (1, 2, 3), ((False, 4), (True, 1)), (3, (256,), 0)),
    ("deep", 512, 8, (32,), ((False, 16), (False, 1)), (2, (128,), 0)),
    ("wide form 1", 1024, 4, (64,), ((False, 32), (False, 1)), (4, (128,), 1)),
    ("wide form 2", 512, 8, (64,), ((False, 16),), (4, (256,), 2)),
    ("wide form 3", 2048, 2, (64,), ((False, 64),), (4, (64,), 3)),
]
STRIP = [(128, 32, ((False, 4), (False, 1), (True, 4))), (256, 16, ((False, 8), (True, 1)))]
UNFUSED = [(128, 32, 32), (128, 64, 4)]                          # (C, side, stats_np): 32 partials keep (128, 32) off the strip form


def _fp32_rule(got, v64, v32):
    """(max-abs error, the fp32 evaluation's, rel-L2) of an fp32 output against float64; NaN counts as inf."""
    d = (got.double() - v64).abs()
    d = torch.where(d == d, d, torch.full_like(d, float("inf")))
    return float(d.max()), float((v32.double() - v64).abs().max()), float(d.norm() / v64.norm().clamp_min(1e-30))


def _g_rule(S, got, g64, g32, faces, side, where):
    """The bf16 rule on G, element by element, with the worst face and pixel class named.  Returns the worst excess (<= 1 passes)."""
    import forced
    import gemm_ref as G
    e32 = float((g32.double() - g64).abs().max())
    ulp = G.bf16_ulp(g64.abs() + forced.F64_MARGIN * e32)
    ex = ((got.double() - g64).abs() - ulp / 2) / (forced.F64_MARGIN * e32 if e32 > 0 else 1e-300)
    ex = torch.where(ex == ex, ex, torch.full_like(ex, float("inf"))).clamp_min(0.0)
    per_face = ex.reshape(faces, -1).max(1).values
    cls = S.CR.pixel_class(side).repeat(faces)
    per_class = {S.CR.PIXEL_CLASSES[k]: float(ex[cls == k].max()) for k in sorted(set(cls.tolist()))}
    worst, wface, wcls = float(ex.max()), int(per_face.argmax()), max(per_class, key=per_class.get)
    print(f"{where}: G excess {worst:.3f} of {forced.F64_MARGIN} x {e32:.3e}; worst face {wface}; worst pixels {wcls} {per_class}")
    assert worst <= 1.0, f"{where}: G beyond ulp / 2 + {forced.F64_MARGIN} x {e32:.3e} by a factor {worst:.3g}; worst face {wface}, worst pixels {wcls} {per_class}"
    return worst, wface, wcls


def dw_reference(S, C, side, faces, stats_np, per_face, seed=0):
    CR = S.CR
    full = CR.make_dw_operands(C, side, faces, stats_np, per_face=per_face, face0=3 if per_face else 0, seed=seed)
    W = S.R.dw_weight(C)
    import gemm_ref as G
    if not torch.equal(G.a_operand(full).float(), G.a_operand(full, torch.float32)):
        pytest.fail("input error: elements of the LayerNorm operand round differently in fp32 and float64")
    return full, CR.evaluate_dw(full, *W), CR.evaluate_dw(full, *W, dtype=torch.float32)


def check_dw(S, full, r64, r32, faces, label, path):
    """One HD_CONV_DWGATE launch of the first `faces` faces, twice, and every assertion that applies to the form that ran."""
    import forced
    CR, R = S.CR, S.R
    ops = CR.dw_slice(full, faces)
    C, side, hw, M = ops["C"], ops["side"], ops["hw"], ops["M"]
    rc, note, got = R.launch_dw(ops)
    assert rc == 0, (label, faces, R.error())
    rc2, _, again = R.launch_dw(ops)
    assert rc2 == 0, (label, faces, R.error())
    where = f"{label} faces {faces} np {ops['stats_np']} [{CR.dw_note_key(ops, note)}]"
    if note["dw_path"] != path:
        pytest.fail(f"input error: {where} took path {note['dw_path']}, not {path}")
    xin, sin = got.pop("_x"), got.pop("_stats")
    again.pop("_x"), again.pop("_stats")
    assert CR.same_bits(xin[:M], ops["A"].bfloat16()) and CR.untouched(xin[M:]) and CR.untouched(sin[M:]), f"{where}: an input changed"
    nb, ns = (side + 7) // 8, side // 4
    used = {"G": M, "pooled": 0 if path == 2 else faces, "pooled16": faces if path == 1 else 0,
            "T1": 0 if path == 1 else faces * ns if path == 2 else 2 * M + faces * nb}
    for k, t in got.items():
        assert CR.untouched(t[used[k]:]), f"{where}: {k} written past row {used[k]}"
        assert CR.same_bits(t, again[k]), f"{where}: {k} differs between two launches"
    g64, g32, p64, p32 = r64["g"][:M], r32["g"][:M], r64["pooled"][:faces], r32["pooled"][:faces]
    t1_ratio = 0.0
    if path == 3:                                                # conv1's T1 under the GEMM rule, everything behind it from the stored T1
        t1 = got["T1"][:2 * M].reshape(M, 2 * C)
        err, e32, rel = _fp32_rule(t1, r64["t1"][:M], r32["t1"][:M])
        t1_ratio = err / e32 if e32 > 0 else float("inf")
        print(f"{where}: T1 maxabs {err:.3e} torch fp32 {e32:.3e} ratio {t1_ratio:.2f} rel {rel:.3e}")
        assert err <= forced.F64_MARGIN * e32 and rel <= forced.FP32_BOUND, f"{where}: T1 maxabs {err:.3e} vs torch fp32 {e32:.3e}, rel {rel:.3e}"
        w2, b2 = R.dw_weight(C)[2:]
        g64, p64 = CR.depthwise_gate(t1.double(), w2, b2, faces, side)
        g32, p32 = CR.depthwise_gate(t1, w2, b2, faces, side)
    excess, wface, wcls = _g_rule(S, got["G"][:M], g64, g32, faces, side, where)
    if path == 1:
        pooled = got["pooled"][:faces]
        assert CR.same_bits(got["pooled16"][:faces], pooled.bfloat16()), f"{where}: pooled16 is not the bf16 rounding of the stored pooled"
    elif path == 2:                                              # strip sums [face][side / 4][C]: added up here in float64
        pooled = got["T1"][:faces * ns].double().reshape(faces, ns, C).sum(1) / hw
    else:                                                        # band sums [face][bands][C] against float64, pool_finish on them bit for bit
        bands = got["T1"][2 * M:2 * M + faces * nb].reshape(faces, nb, C)
        pad = lambda g: torch.cat((g.reshape(faces, side, side, C), torch.zeros(faces, nb * 8 - side, side, C, dtype=g.dtype)), 1)      # noqa: E731
        b64, b32 = (pad(g).reshape(faces, nb, 8 * side, C).sum(2) for g in (g64, g32))
        err, e32, rel = _fp32_rule(bands, b64, b32)
        print(f"{where}: band sums maxabs {err:.3e} torch fp32 {e32:.3e} rel {rel:.3e}")
        assert err <= forced.F64_MARGIN * e32 and rel <= forced.FP32_BOUND, f"{where}: band sums maxabs {err:.3e} vs torch fp32 {e32:.3e}, rel {rel:.3e}"
        acc = torch.zeros(faces, C)
        for b in range(nb):
            acc = acc + bands[:, b]
        assert CR.same_bits(got["pooled"][:faces], acc * torch.tensor(1.0 / hw, dtype=torch.float32)), f"{where}: pooled is not the band sums added in band order x 1 / HW"
        pooled = got["pooled"][:faces]
    err, e32, rel = _fp32_rule(pooled, p64, p32)
    pf = (pooled.double() - p64).norm(dim=1) / p64.norm(dim=1).clamp_min(1e-30)
    p_ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{where}: pooled maxabs {err:.3e} torch fp32 {e32:.3e} ratio {p_ratio:.2f} rel {rel:.3e}; worst face {int(pf.argmax())} rel {float(pf.max()):.3e}")
    assert err <= forced.F64_MARGIN * e32 and rel <= forced.FP32_BOUND and float(pf.max()) <= forced.FP32_BOUND, \
        f"{where}: pooled maxabs {err:.3e} vs torch fp32 {e32:.3e}, rel {rel:.3e}, worst face {int(pf.argmax())} rel {float(pf.max()):.3e}"
    w = S.dw_worst.setdefault(CR.dw_note_key(ops, note), [0.0, 0.0, 0.0, 0, 0, ""])
    if excess >= w[0]:
        w[4], w[5] = wface, wcls
    w[0], w[1], w[2], w[3] = max(w[0], excess), max(w[1], p_ratio), max(w[2], t1_ratio), w[3] + 1
    return note


@pytest.mark.parametrize("case", FUSED, ids=[c[0] for c in FUSED])
def test_fused_depthwise_gate_on_every_dispatch_branch(S, case):
    """LayerNorm + FiLM -> conv1 -> depthwise 3x3 -> SimpleGate -> G, pooled, pooled16 in one launch: EpDwGate1 (one pixel per face) and every
    branch of dispatch_dwgate -- skinny <1,1>, <1,2>, <2,1>, <8,1> for 8 x 8 and for 16 x 16 faces, the deep and the wide kernel -- each
    at the smallest M at which the library gives it, with a face short of a full tile where the rule allows one, shared and per-face
    FiLM rows, the partials as 1 x C and C / 32 x 32.  The dry run confirms the form, the note the branch.  G under the bf16 rule,
    pooled under the fp32 rule and per face, pooled16 the rounding of pooled.  Measured (profiles/r26_conv_edges.txt): G beyond half an ulp by at
    most 0.061 of the allowed 4 x e32 (wide form 3), pooled at most 2.56 x torch's fp32 error (skinny <2,1>; deep 1.11, wide <= 1.66)."""
    cid, C, side, counts, variants, (fam, rows, form) = case
    for per_face, np_ in variants:
        full, r64, r32 = dw_reference(S, C, side, max(counts), np_, per_face, seed=len(cid))
        for faces in counts:
            ops = S.CR.dw_slice(full, faces)
            rc, dry, _ = S.R.launch_dw(ops, dry=True)
            assert rc == 0, S.R.error()
            if dry["dw_path"] != 1:
                pytest.fail(f"input error: {cid} at {faces} faces is given path {dry['dw_path']}, not the fused form")
            note = check_dw(S, full, r64, r32, faces, f"dwgate {cid} C {C} side {side}{' per-face' if per_face else ''}", 1)
            g = note["gemm"]
            if g["family"] != fam or g["rows"] not in rows or g["wide_form"] != form:
                pytest.fail(f"input error: {cid} at {faces} faces ran family {g['family']} rows {g['rows']} form {g['wide_form']}, not {fam} {rows} {form}")
            S.dw_seen.add((cid, per_face, np_ == 1, (faces * side * side) % g["rows"] != 0))


@pytest.mark.parametrize("C,side,variants", STRIP, ids=[f"C{c}-side{s}" for c, s, _ in STRIP])
def test_depthwise_gate_by_strips(S, C, side, variants):
    """(128, 32) and (256, 16) at 1, 2 and 3 faces: G under the bf16 rule; the strip leaves [face][side / 4][C] sums, added up here in float64
    and held to the same mean under the fp32 rule; pooled and pooled16 stay untouched.  Measured (profiles/r26_conv_edges.txt): G excess <= 0.043,
    the summed strips at most 2.98 x torch's fp32 error (C 128), 1.48 (C 256)."""
    for per_face, np_ in variants:
        full, r64, r32 = dw_reference(S, C, side, 3, np_, per_face, seed=5)
        for faces in (1, 2, 3):
            check_dw(S, full, r64, r32, faces, f"dwgate strip C {C} side {side}{' per-face' if per_face else ''}", 2)
            S.dw_seen.add((f"strip {C} {side}", per_face, np_ == 1, False))


@pytest.mark.parametrize("C,side,np_", UNFUSED, ids=[f"C{c}-side{s}" for c, s, _ in UNFUSED])
def test_unfused_depthwise_gate_and_pool_finish(S, C, side, np_):
    """(128, 32) (with 32 partials, which the strip form does not take) and (128, 64) at 1 and 2 faces: conv1's T1 under the GEMM rule; from
    the T1 the kernel stored, G under the bf16 rule and the band sums under the fp32 rule; pooled bit for bit the band sums added in
    band order times 1 / HW, and under the fp32 rule against the mean.  Measured (profiles/r26_conv_edges.txt): T1 <= 0.95 x torch's fp32 error,
    band sums <= 1.2 x, G excess <= 0.044, pooled <= 1.00 x."""
    full, r64, r32 = dw_reference(S, C, side, 2, np_, False, seed=6)
    for faces in (1, 2):
        check_dw(S, full, r64, r32, faces, f"dwgate unfused C {C} side {side}", 3)
        S.dw_seen.add((f"unfused {C} {side}", False, False, False))


def test_refusals_return_invalid_and_launch_nothing(S):
    """Everything the entry does not take is HD_ERR_INVALID with a message that names the field, and no output byte changes."""
    import ctypes
    CR, R = S.CR, S.R
    R.weight("hca", 128), R.weight("down", 128)
    R.load("nobias", torch.zeros(128, 128, 3, 3), None)
    x = CR.make_input(2, 4, 128)

    def bump(field, by):
        return lambda d: setattr(d, field, (getattr(d, field) or 0) + by)

    def put(field, v):
        return lambda d: setattr(d, field, v)

    cases = [
        ("hca", put("side", 3), None, "side = 3"), ("hca", put("side", 0), None, "side = 0"), ("hca", put("side", 64), None, "side = 64"),
        ("down", put("side", 1), None, "side = 1"), ("hca", put("M", 31), None, "M = 31"), ("hca", put("M", 0), None, "M = 0"),
        ("down", put("M", 40), None, "M = 40"), ("hca", put("C", 48), None, "C = 48"), ("hca", put("C", 0), None, "C = 0"),
        ("hca", put("C", 4096), None, "C = 4096"), ("hca", put("M", 65552), None, "M = 65552"),
        ("hca", put("X", None), None, "X is"), ("hca", bump("X", 2), None, "X is"), ("hca", put("out", None), None, "out is"),
        ("down", bump("out", 8), None, "out is"), ("hca", bump("out16", 2), None, "out16 is"), ("down", bump("stats_out", 8), None, "stats_out is"),
        ("hca", put("stats_out", 4096), None, "stats_out is"),
        ("hca", None, "down128", "down128.weight"), ("down", None, "hca128", "hca128.weight"), ("hca", put("C", 256), None, "hca128.weight"),
        ("hca", None, "nothing", "nothing.weight"), ("hca", None, "nobias", "nobias.bias"),
    ]
    for kind, edit, name, field in cases:
        rc, note, got = R.launch(kind, x, 128, 4, edit=edit, name=name)
        assert rc == HD_ERR_INVALID and field in R.error(), (field, rc, R.error())
        got.pop("_x")
        assert note["form"] == 0 and all(CR.untouched(t) for t in got.values()), field
    _lib, L = R._lib, R.L
    d, note = _lib.ConvDesc(), _lib.ConvNote()
    buf = torch.zeros(64 * 128, device="cuda")
    d.M, d.C, d.side, d.X, d.out = 32, 128, 4, buf.data_ptr(), buf.data_ptr()
    for kind, w2, field in ((3, None, "kind"), (-1, None, "kind"), (0, b"hca128", "weight2"), (2, None, "weight2")):
        assert L.hd_debug_conv(R.ctx, kind, b"hca128", w2, ctypes.byref(d), 0, ctypes.byref(note), None) == HD_ERR_INVALID and field in R.error(), R.error()
    assert L.hd_debug_conv(R.ctx, 0, b"hca128", None, None, 0, ctypes.byref(note), None) == HD_ERR_INVALID and "desc" in R.error(), R.error()
    # the depthwise kind
    ops = CR.make_dw_operands(128, 4, 2, 4, per_face=True, face0=3)
    R.dw_weight(128)
    dw_cases = [
        (put("side", 3), None, "side = 3"), (put("side", 128), None, "side = 128"), (put("M", 31), None, "M = 31"), (put("C", 48), None, "C = 48"),
        (put("stats_np", 3), None, "stats_np"), (put("stats_cnt", 16), None, "stats_cnt"), (put("film_off", 6), None, "film_off"),
        (put("film_face_stride", 6), None, "film_face_stride"), (put("face0", -1), None, "face0"), (put("T1_elems", 100), None, "T1_elems"),
        (put("X", None), None, "X is"), (bump("stats_in", 8), None, "stats_in is"), (put("film", None), None, "film is"), (bump("G", 2), None, "G is"),
        (put("pooled", None), None, "pooled is"), (bump("pooled16", 2), None, "pooled16 is"), (put("T1", None), None, "T1 is"),
        (put("out", 4096), None, "out, out16 and stats_out"), (None, ("hca128", "dwc128"), "hca128.weight"), (None, ("dw128", "dw128"), "dw128.weight"),
        (None, ("dw128", "nothing"), "nothing.weight"),
    ]
    for edit, names, field in dw_cases:
        rc, note2, got = R.launch_dw(ops, edit=edit, names=names)
        assert rc == HD_ERR_INVALID and field in R.error(), (field, rc, R.error())
        got.pop("_x"), got.pop("_stats")
        assert note2["form"] == 0 and all(CR.untouched(t) for t in got.values()), field
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0
    assert not [n for n in R.notes if n[1] == 128 and n[2] == 4 and n[0] != "dw"] and not [n for n in R.notes if n[0] == "dw" and n[1:4] == (128, 4, 2)]


def test_the_cases_cover_every_kernel_path(S):
    """The coverage conditions, on the launch notes of the tests above (this test runs after them): every staged ConvCfg, fewer faces than
    a workgroup holds, a ragged last workgroup, the XCD remap with a ragged row group, the gather and centre-only forms, every down-conv,
    the 32-row hint, a ragged last row tile of the gather kernels; EpDwGate1 and every branch of dispatch_dwgate with shared and per-face
    FiLM rows and both forms of the partials, a ragged last tile where the branch's rule allows one, the strip form and the unfused pair.
    A failure means the cases are the wrong ones, not that a kernel is.  Prints the report (worst figures per kernel note) and the
    module's wall time."""
    CR, notes = S.CR, S.R.notes
    miss = []
    for (C, side), (bm, ks, nt, strip) in CR.STAGED.items():
        mine = [(f, n) for k, c, s, f, n in notes if k == "hca" and (c, s) == (C, side) and n["form"] == 1 and (n["bm"], n["ks"], n["nt"], n["strip"]) == (bm, ks, nt, strip)]
        fpw = CR.faces_per_workgroup(C, side)
        if not mine:
            miss.append(f"staged conv C {C} side {side}")
        if fpw > 1 and not any(f % fpw != 0 and f > fpw for f, n in mine):
            miss.append(f"staged conv C {C} side {side}: a ragged last workgroup behind a full one")
        if fpw > 1 and not any(f < fpw for f, n in mine):
            miss.append(f"staged conv C {C} side {side}: fewer faces than one workgroup holds")
        if C >= 1024 and not any(n["remap"] and n["grid_x"] == 2 and f % fpw != 0 for f, n in mine):
            miss.append(f"staged conv C {C} side {side}: the XCD remap with a ragged row group")
        if not any(n["grid_x"] > 1 for f, n in mine):
            miss.append(f"staged conv C {C} side {side}: more than one row group")
    for C, side, _ in GATHER:
        if not any(k == "hca" and (c, s) == (C, side) and n["form"] == 2 and n["centre_only"] == (side == 1) for k, c, s, f, n in notes):
            miss.append(f"gather C {C} side {side}")
    for C, side, _ in DOWN:
        if not any(k == "down" and (c, s) == (C, side) and n["form"] == 2 for k, c, s, f, n in notes):
            miss.append(f"down C {C} side {side}")
    if not any(k == "down" and n["hint"] == 3 for k, c, s, f, n in notes):
        miss.append("down-conv with the 32-row hint")
    for kind in ("hca", "down"):                                 # a ragged last row tile of the gather kernels
        if not any(k == kind and n["form"] == 2 and (f * s * s // (4 if k == "down" else 1)) % n["gemm"]["rows"] != 0 for k, c, s, f, n in notes):
            miss.append(f"{kind} gather with a ragged last row tile")
    for cid, C, side, counts, variants, _ in FUSED:
        mine = [x for x in S.dw_seen if x[0] == cid]
        if not mine:
            miss.append(f"fused depthwise: {cid}")
        for per_face, np_ in variants:
            if not any(x[1] == per_face and x[2] == (np_ == 1) for x in mine):
                miss.append(f"fused depthwise: {cid}{' per-face' if per_face else ''} np {np_}")
        if (cid == "EpDwGate1" or cid.startswith("skinny<1,1>")) and not any(x[3] for x in mine):      # the other branches need M % rows == 0
            miss.append(f"fused depthwise: {cid} with a ragged last tile")
    for want in ("deep", "wide form 1"):
        if not any(x[0] == want for x in S.dw_seen):
            miss.append(f"dispatch_dwgate branch {want}")
    if not any(x[1] for x in S.dw_seen) or not any(not x[1] for x in S.dw_seen):
        miss.append("shared and per-face FiLM rows")
    for C, side, _ in STRIP:
        if not any(k == "dw" and (c, s) == (C, side) and n["dw_path"] == 2 for k, c, s, f, n in notes):
            miss.append(f"strip form C {C} side {side}")
    for C, side, _ in UNFUSED:
        if not any(k == "dw" and (c, s) == (C, side) and n["dw_path"] == 3 for k, c, s, f, n in notes):
            miss.append(f"unfused form C {C} side {side}")
    print(f"{'depthwise kernel note':64s} {'n':>4s} {'G excess':>9s} {'pooled ratio':>12s} {'T1 ratio':>9s}  worst face, pixels")
    for key, (ex, pr, tr, n, wf, wc) in sorted(S.dw_worst.items()):
        print(f"{key:64s} {n:4d} {ex:9.3f} {pr:12.2f} {tr:9.2f}  {wf} {wc}")
    print(f"{len(notes)} launches in {time.time() - S.t0:.1f} s (module wall time so far), worst stats_out error {S.stat_worst:.3e}")
    print(f"{'kernel note':64s} {'n':>4s} {'fp32 maxabs':>12s} {'torch fp32':>11s} {'ratio':>6s} {'sliced':>6s} {'bf16 excess':>11s}  worst face (rel, face, pixels)")
    for key, (ratio, (err, e32), excess, n, sliced) in sorted(S.worst.items()):
        print(f"{key:64s} {n:4d} {err:12.3e} {e32:11.3e} {ratio:6.2f} {sliced:6.2f} {excess:11.3f}  {S.faces.get(key)}")
    if miss:
        pytest.fail("input error: the cases do not reach " + "; ".join(miss))
