"""The shared GEMM kernels (hd_gemm.hpp, hd_wide.hpp) one launch at a time against float64, at the tile and batch edges the network
scans do not sit on.  Every launch goes through `hd_debug_gemm`, i.e. through the library's own add_gemm: kernel mode, half tiles, K
split, straight-line or run-time K loop, w_nt, xcd_tile_affine, the deep and the wide kernel are chosen by the library from (M, N, K),
never forced, and what ran is read from the launch note.  Operands, reference and runner: tools/gemm_ref.py (held against torch without
a GPU by tests/test_gemm_ref_host.py).

Per launch: fp32 outputs max-abs against float64 <= forced.F64_MARGIN x the max-abs error of the same evaluation in torch fp32 on the
CPU (exactly 0 where that is 0) and rel-L2 <= forced.FP32_BOUND; bf16 outputs elementwise |got - v64| <= ulp_bf16 / 2 + F64_MARGIN x e32
(ulp of the larger-magnitude neighbour at a binade edge; e32: the fp32 evaluation's max-abs error of the unrounded value), out16 bit
for bit the bf16 rounding of the fp32 `out` the kernel stored; stats_out under forced.Check's statistics rule at STAT_BOUND; 64 guard
rows behind every output (behind 4 M rows for PixelShuffle r = 2) and, with ldo = N + 32, the pad columns still hold the NaN pattern
they were filled with; a second launch gives the same bits.

N: 128 (plain) / 256 (pair) in the small-tile cases.  No N that is not a multiple of 32: among the three launch programs the only
GEMMs with such an N are patch-gather convolutions (the VAE's conv_out with N = 8 / 3, CoarseRestoration's STN localization convs),
whose LK_CONV_* loaders need face images and stay with the network scans; every GEMM of the nine families here has whole 32-column
tiles.  Figures: profiles/r21_gemm_edges.txt."""
import os
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

SMALL_M = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 255, 256, 257)
FACE_M = tuple(m for m in SMALL_M if m % 16 == 0)                # hw = 4, Win = 4
PAD_M = (17, 64, 257)                                            # the row-major epilogues once more with ldo = N + 32
KS = (128, 256, 512, 1024, 2048)
F32_KS = (32, 96) + KS                                           # K != Kp: the run-time K loop (CoarseRestoration level 0)
HD_ERR_INVALID = -1

# (id, family, N, K, operand kwargs, ((M, expected base mode or None, expected extra bits, launch kwargs), ...)): the smallest M at which
# add_gemm itself gives the kernel (choose_mode, deep_shape_ok, wide_shape_ok as they stand), confirmed by the dry run
T = lambda ms: tuple((m, md, 0, {}) for m, md in ms)             # noqa: E731
TALL_MS = T(((8129, 1), (16257, 0), (16352, 0), (16353, 4)))
LARGE = [
    ("tall-f32", "f32_biasf32", 128, 128, dict(act=1), TALL_MS),
    ("tall-bf16-resid", "bf16_resid", 128, 128, {}, TALL_MS),
    ("tall-ln", "ln_biasf32", 128, 128, dict(stats_np=4), TALL_MS),
    ("tall-ln-pair", "ln_gate", 256, 128, dict(stats_np=1), TALL_MS),
    ("tall-ln-pair-face", "ln_gate", 256, 128, dict(stats_np=4, per_face=True, hw=1, face0=3), TALL_MS[:2]),
    ("mode2-bf16-resid", "bf16_resid", 1024, 1024, {}, T(((321, 2),))),
    ("mode2-bf16-biasbf16", "bf16_biasbf16", 1024, 1024, dict(act=1), T(((321, 2),))),
    ("mode2-ln-pair", "ln_gate", 2048, 1024, dict(stats_np=32), T(((321, 2),))),
    ("mode5-bf16s", "bf16s_resid", 512, 1024, dict(hw=1), T(((2048, 5), (2049, 5)))),
    ("mode5-bf16-biasf32", "bf16_biasf32", 512, 1024, {}, T(((2048, 5), (2049, 5)))),
    ("mode5-ln-pair-face", "ln_gate", 1024, 1024, dict(stats_np=32, per_face=True, hw=1, face0=3), T(((2048, 5), (2049, 5)))),
    ("mode6-bf16s", "bf16s_resid", 1024, 1024, dict(hw=1), T(((2048, 6), (2303, 6)))),
    ("mode6-f32-pixshuf", "f32_pixshuf", 1024, 1024, {}, T(((2048, 6), (2303, 6)))),
    ("mode6-ln-pair-face", "ln_gate", 2048, 1024, dict(stats_np=32, per_face=True, hw=1, face0=3), T(((2048, 6), (2303, 6)))),
    # the deep kernel; at M = 1024, K = 1024 the wide kernel comes first unless lda != K
    ("deep-pair-k1024", "ln_gate", 2048, 1024, dict(stats_np=32), ((1024, None, 16, dict(lda_pad=8)), (1025, None, 16, {}))),
    ("deep-pair-k1024-np1", "ln_gate", 2048, 1024, dict(stats_np=1), ((1025, None, 16, {}),)),
    ("deep-pair-k512", "ln_gate", 2048, 512, dict(stats_np=16), ((1024, None, 16, {}), (1025, None, 16, {}))),
    ("deep-plain-k512", "bf16_resid", 512, 512, {}, ((2048, None, 16, {}), (2049, None, 16, {}))),
    ("deep-plain-k1024", "bf16_resid", 512, 1024, {}, ((2049, None, 16, {}),)),
    ("wide1-ln-pair", "ln_gate", 2048, 1024, dict(stats_np=32), ((1024, None, 32, {}),)),
    ("wide1-ln-pair-np1", "ln_gate", 2048, 1024, dict(stats_np=1), ((1024, None, 32, {}),)),
    ("wide1-bf16-plain", "bf16_resid", 1024, 1024, {}, ((1024, None, 32, {}),)),
    ("wide3-ln-pair", "ln_gate", 1024, 2048, dict(stats_np=64), ((1024, None, 32, {}),)),
]
SHAPES = {(128, k) for k in F32_KS} | {(256, k) for k in KS} | {(c[2], c[3]) for c in LARGE}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


class State:
    def __init__(self, G):
        self.G, self.R = G, G.Runner(SHAPES)
        self.worst = {}                                          # (family, note key) -> [fp32 ratio, (err, e32), bf16 excess, launches]
        self.ragged = set()                                      # (family, kernel family) with M % rows != 0
        self.moved, self.stat_worst = 0, 0.0


@pytest.fixture(scope="module")
def S(gpu):
    import gemm_ref as G
    s = State(G)
    yield s
    s.R.close()


# ---------------------------------------------------------------------------------------------- the checks of one launch
def _bf16_rule(G, got, v64, e32, margin):
    """max over the elements of (|got - v64| - ulp / 2) / (margin * e32) (<= 1 passes; e32 = 0: any excess is inf)."""
    ulp = G.bf16_ulp(v64.abs() + margin * e32)
    excess = (got.double() - v64).abs() - ulp / 2
    if not bool((excess == excess).all()):
        return float("inf")
    worst = float(excess.max())
    return 0.0 if worst <= 0 else (worst / (margin * e32) if e32 > 0 else float("inf"))


def check_launch(S, full, ref, M, label, launch_kw=None):
    """Launches the first M rows of `full` twice and applies every assertion of the module docstring.  Returns the note."""
    import forced
    G, R = S.G, S.R
    fam = full["family"]
    ek = G.FAMILIES[fam][1]
    ops = dict(G.slice_rows(full, M), **(launch_kw or {}))
    rc, note, got = R.launch(ops, full)
    assert rc == 0, (label, M, R.error())
    rc2, _, again = R.launch(ops, full)
    assert rc2 == 0, (label, M, R.error())
    rows = 4 * M if ops["shuffle_r"] == 2 else M
    v64, v32 = ref[0]["v"][:rows], ref[1]["v"][:rows].double()
    ncols = v64.shape[1]
    e32 = float((v32 - v64).abs().max())
    where = f"{label} M {M} [{G.note_key(note)}]"
    for k, t in got.items():                                     # guards, pad columns, the repeat launch
        w = 2 * (ncols // 32) if k == "stats_out" else ncols
        assert G.untouched(t[rows:]), f"{where}: {k} written past row {rows}"
        assert G.untouched(t[:rows, w:]), f"{where}: {k} pad columns written"
        assert G.same_bits(t, again[k]), f"{where}: {k} differs between two launches"
    body = got["out"][:rows, :ncols]
    ratio = excess = 0.0
    err = float("nan")
    if ek in G.BF16_OUT:
        excess = _bf16_rule(G, body, v64, e32, forced.F64_MARGIN)
        assert excess <= 1.0, f"{where}: bf16 out beyond ulp / 2 + {forced.F64_MARGIN} x {e32:.3e} by a factor {excess:.3g}"
    else:
        d = body.double() - v64
        err, rel = float(d.abs().max()), float(d.norm() / v64.norm().clamp_min(1e-30))
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        print(f"{where}: maxabs {err:.3e} torch fp32 {e32:.3e} ratio {ratio:.2f} rel {rel:.3e}")
        assert err <= forced.F64_MARGIN * e32 and rel <= forced.FP32_BOUND, f"{where}: maxabs {err:.3e} vs torch fp32 {e32:.3e}, rel {rel:.3e}"
        if "out16" in got:
            o16 = got["out16"][:rows, :ncols]
            assert G.same_bits(o16, body.bfloat16()), f"{where}: out16 is not the bf16 rounding of the stored out"
            excess = max(excess, _bf16_rule(G, o16, v64, e32, forced.F64_MARGIN))
        if "stats_out" in got:
            rep = []
            ck = forced.Check(rep)
            me, re_, _ = ck.stats(0, label, "stats_out", got["stats_out"][:rows].reshape(-1), body, ncols // 32, 32)
            S.stat_worst = max(S.stat_worst, me, re_)
            assert me <= forced.STAT_BOUND and re_ <= forced.STAT_BOUND, f"{where}: {rep[-1]}"
        if "outg16" in got:
            g64 = ref[0]["g"][:rows]
            e32g = float((ref[1]["g"][:rows].double() - g64).abs().max())
            excess = max(excess, _bf16_rule(G, got["outg16"][:rows, :ncols], g64, e32g, forced.F64_MARGIN))
        assert excess <= 1.0, f"{where}: a bf16 output beyond ulp / 2 + {forced.F64_MARGIN} x the fp32 error by a factor {excess:.3g}"
    key = (fam, G.note_key(note))
    w = S.worst.setdefault(key, [0.0, (0.0, 0.0), 0.0, 0])
    if ratio >= w[0] and err == err:
        w[0], w[1] = ratio, (err, e32)
    w[2], w[3] = max(w[2], excess), w[3] + 1
    if M % note["rows"] != 0:
        S.ragged.add((fam, note["family"]))
    return note


def _reference(S, full, N, K):
    fw = S.R.with_weight(full, N, K)
    if "moved" in full:
        S.moved += full["moved"]
        a64, a32 = S.G.a_operand(fw), S.G.a_operand(fw, torch.float32)
        if not torch.equal(a64.float(), a32):
            pytest.fail(f"input error: {int((a64.float() != a32).sum())} elements of the A operand round differently in fp32 and float64")
        import cr_forced
        if "ratio" in full and not float(full["ratio"][3::4].min()) >= cr_forced.RATIO_MIN:
            pytest.fail(f"input error: offset rows reach |row mean| / row std {float(full['ratio'][3::4].min()):.1f} < {cr_forced.RATIO_MIN}")
    return fw, (S.G.evaluate(fw), S.G.evaluate(fw, torch.float32))


def _variants(family, K):
    """(label, make_operands kwargs, the M values) of the small-tile cases of a family."""
    lk, ek = family.split("_")
    out = []
    if lk == "ln":
        for np_ in (1, K // 32):                                 # the two forms the programs produce
            out.append((f"shared np {np_}", dict(stats_np=np_), SMALL_M))
            out.append((f"per-face np {np_}", dict(stats_np=np_, per_face=True, hw=4, face0=3), FACE_M))
        out.append(("shared ldo+32", dict(stats_np=K // 32, ldo_pad=32), PAD_M))
        return out
    act = dict(act=2 if K < 128 else 1) if family == "f32_biasf32" else dict(act=1) if ek == "biasbf16" else {}      # sigmoid, ReLU
    out.append(("hw 1", dict(act), SMALL_M))
    if lk == "bf16s":
        out.append(("hw 4", dict(hw=4), FACE_M))
    if family == "bf16_resid":
        out.append(("gated hw 4", dict(hw=4, gated=True), FACE_M))
    if ek == "pixshuf":
        out.append(("r 2", dict(shuffle_r=2, win=4), FACE_M))
    out.append(("ldo+32", dict(act, ldo_pad=32), PAD_M))
    return out


def _small_cases():
    fams = ("f32_biasf32", "f32_pixshuf", "bf16_resid", "bf16s_resid", "bf16_biasbf16", "bf16_pixshuf", "bf16_biasf32", "ln_gate", "ln_biasf32")
    return [(f, k) for f in fams for k in (F32_KS if f.startswith("f32") else KS)]


@pytest.mark.parametrize("family,K", _small_cases())
def test_small_tiles_against_float64(S, family, K):
    """M in {1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 255, 256, 257} with hw = 1, the multiples of 16 again with hw = 4 where rows
    are mapped to faces (BF16S, per-face LayerNorm with face0 = 3 and distinct FiLM rows per face, RESID's outg16) and as 4 x 4 images for
    PixelShuffle r = 2; the LayerNorm partials as 1 x K and K / 32 x 32; M in {17, 64, 257} once more with ldo = N + 32.
    Measured (profiles/r21_gemm_edges.txt), worst max-abs error as a multiple of torch's fp32 error (bound 4): f32_biasf32 1.36,
    f32_pixshuf 1.41, bf16_resid 1.53, bf16s_resid 1.67, bf16_pixshuf 1.39, bf16_biasf32 1.47, ln_biasf32 1.31; rel-L2 <= 1.2e-7 everywhere;
    bf16 outputs beyond half an ulp by at most 0.12 of the allowed 4 x e32 (out16, outg16, BIASBF16, GATE); stats_out <= 1.5e-6; no guard
    row, pad column or repeat launch differed."""
    G = S.G
    N = 256 if family == "ln_gate" else 128
    for label, kw, ms in _variants(family, K):
        full = G.make_operands(family, N, K, max(ms), seed=len(label), **kw)
        fw, ref = _reference(S, full, N, K)
        for M in ms:
            check_launch(S, fw, ref, M, f"{family} N {N} K {K} {label}")


@pytest.mark.parametrize("case", LARGE, ids=[c[0] for c in LARGE])
def test_larger_kernels_at_the_smallest_m_add_gemm_gives_them(S, case):
    """Tall T128 / T64 / T32W, the 64-row skinny tile, the 128 / 256-row M-split workgroups, the deep kernel at K = 512 and 1024 and the
    wide kernel in forms 1 and 3, plain and pair, each at the smallest M choose_mode / deep_shape_ok / wide_shape_ok give it and one
    past a tile edge where the shape rule allows a ragged last tile.  The dry run confirms the pick before anything is launched.
    Measured (profiles/r21_gemm_edges.txt), worst max-abs error as a multiple of torch's fp32 error (bound 4): the deep kernel at
    K = 1024 2.76, the 256-row M-split workgroup (one wave sums all of K = 1024) 2.51 / 2.30, tall tiles <= 1.0; the pair kernels'
    bf16 output beyond half an ulp by at most 0.29 of the allowed 4 x e32 (256-row workgroups, per-face LayerNorm)."""
    G = S.G
    cid, family, N, K, kw, picks = case
    full = G.make_operands(family, N, K, max(p[0] for p in picks), seed=7, **kw)
    fw, ref = _reference(S, full, N, K)
    for M, base, bits, lkw in picks:
        ops = dict(G.slice_rows(fw, M), **lkw)
        rc, note, _ = S.R.launch(ops, fw, dry=True)
        assert rc == 0, S.R.error()
        if (base is not None and note["mode"] != base) or (note["mode"] & 48 & bits) != bits or (base is not None and note["mode"] & 48):
            pytest.fail(f"input error: {cid} at M = {M} is given mode {note['mode']}, not {base if base is not None else ''}+{bits}")
        note = check_launch(S, fw, ref, M, f"{cid} {family} N {N} K {K}", lkw)
        want = 4 if bits == 32 else 2 if bits == 16 else (1 if base in (0, 1, 4) else 3)
        if note["family"] != want:
            pytest.fail(f"input error: {cid} at M = {M} ran kernel family {note['family']}, not {want}")


def test_refusals_return_invalid_and_launch_nothing(S):
    """Everything the packer or a launcher does not take is HD_ERR_INVALID with a message that names the field, and no output changes."""
    G, R = S.G, S.R
    full = R.with_weight(G.make_operands("ln_biasf32", 128, 128, 32, stats_np=4, per_face=True, hw=4, face0=3), 128, 128)
    plain = R.with_weight(G.make_operands("bf16s_resid", 128, 128, 32, hw=4), 128, 128)
    shuf = R.with_weight(G.make_operands("f32_pixshuf", 128, 128, 32, shuffle_r=2, win=4), 128, 128)
    gate = R.with_weight(G.make_operands("bf16_resid", 128, 128, 32, hw=4, gated=True), 128, 128)

    def bump(field, by=4):
        return lambda d: setattr(d, field, (getattr(d, field) or 0) + by)

    def null(field):
        return lambda d: setattr(d, field, None)

    cases = [
        (full, {}, lambda d: setattr(d, "lda", 120), "lda"),
        (full, {}, null("stats_in"), "stats_in"), (full, {}, bump("film"), "film"), (full, {}, bump("A"), "A"), (full, {}, null("out"), "out"),
        (full, {}, bump("out16", 2), "out16"), (full, {}, bump("stats_out", 8), "stats_out"),
        (full, {}, lambda d: setattr(d, "stats_np", 3), "stats_np"), (full, {}, lambda d: setattr(d, "stats_cnt", 16), "stats_cnt"),
        (full, dict(M=30), None, "hw"), (plain, dict(M=30), None, "hw"), (gate, dict(M=30), None, "hw"),
        (plain, {}, null("rowscale"), "rowscale"), (plain, {}, bump("resid"), "resid"), (plain, {}, null("rscale"), "rscale"),
        (gate, {}, null("gate_c"), "gate_c"), (gate, {}, bump("gate_s"), "gate_s"), (gate, {}, bump("add_src"), "add_src"),
        (shuf, {}, lambda d: setattr(d, "Win", 3), "Win"), (shuf, {}, lambda d: setattr(d, "ldo", 48), "ldo"), (shuf, dict(M=24), None, "Win^2"),
        (plain, {}, lambda d: setattr(d, "ldo", 96), "ldo"), (plain, {}, lambda d: setattr(d, "ldr", 64), "ldr"),
        (plain, {}, lambda d: setattr(d, "shuffle_r", 2), "shuffle_r"), (plain, {}, lambda d: setattr(d, "act", 1), "act"),
        (plain, {}, lambda d: setattr(d, "M", 0), "M"),
    ]
    for ops, over, edit, field in cases:
        rc, note, got = R.launch(dict(G.slice_rows(ops, over.get("M", 32))), ops, edit=edit)
        assert rc == HD_ERR_INVALID and field in R.error(), (field, rc, R.error())
        assert note["family"] == 0 and all(G.untouched(t) for t in got.values()), field
    assert not [n for n in R.notes if n[3] in (30, 24)]
    # a loader / epilogue pair the dispatch does not build, an unknown weight, a K that is no multiple of 8: by hand
    _lib, L = R._lib, R.L
    import ctypes
    d, note = _lib.GemmDesc(), _lib.GemmNote()
    d.M, d.hw, d.shuffle_r, d.lda, d.ldo = 32, 1, 1, 128, 128
    buf = torch.zeros(64 * 128, device="cuda")
    d.A = d.out = buf.data_ptr()
    for lk, ek, name, field in ((3, 4, b"g128x128", "loader"), (0, 2, b"g128x128", "loader"), (2, 0, b"nothing", "weight")):
        assert L.hd_debug_gemm(R.ctx, name, lk, ek, ctypes.byref(d), 0, ctypes.byref(note), None) == HD_ERR_INVALID and field in R.error(), R.error()
    w = torch.randn(32, 20)
    td = _lib.TensorDesc()
    td.name, td.data, td.ndim, td.is_device = b"k20.weight", w.data_ptr(), 2, 0
    td.shape[0], td.shape[1] = 32, 20
    _lib.check(L.hd_load_weights(R.ctx, ctypes.byref(td), 1), R.ctx)
    d.lda = 24
    assert L.hd_debug_gemm(R.ctx, b"k20", 2, 0, ctypes.byref(d), 0, ctypes.byref(note), None) == HD_ERR_INVALID and "K = 20" in R.error(), R.error()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


def test_half_tiles_start_and_stop_where_the_notes_of_the_small_cases_say(S):
    """The 16-row half tile is a matter of speed, not of results, so no bound above sees its threshold move.  On the notes of the small-tile
    cases with K >= 512 (a K split of 4 or 8; runs after them): M = 16, 32, 48 and 64 ran 16-row workgroups, every other M -- 17, 63,
    65, 80 among them -- did not."""
    seen = {}
    for f, n, k, m, np_, pf, nt in S.R.notes:
        if n in (128, 256) and k >= 512 and nt["family"] == 3:
            seen.setdefault(m, set()).add(nt["rows"])
    if not set(SMALL_M) <= set(seen):
        pytest.fail(f"input error: no small-tile launch noted for M in {sorted(set(SMALL_M) - set(seen))}")
    for m in SMALL_M:
        assert seen[m] == ({16} if m <= 64 and m % 16 == 0 else {32}), (m, seen[m])


def test_the_cases_cover_every_kernel_path(S):
    """The coverage conditions, on the launch notes of the tests above (this test runs after them): a failure means the cases are the
    wrong ones, not that a kernel is.  Prints the report (worst figures per family and kernel note)."""
    G, notes = S.G, S.R.notes
    have = lambda pred: any(pred(f, n, k, m, np_, pf, nt) for f, n, k, m, np_, pf, nt in notes)      # noqa: E731
    miss = []
    for rows, name in ((128, "T128"), (64, "T64"), (32, "T32W")):
        for pair in (0, 1):
            if not have(lambda f, n, k, m, np_, pf, nt: nt["family"] == 1 and nt["rows"] == rows and nt["pair"] == pair):
                miss.append(f"tall {name} {'pair' if pair else 'plain'}")
    for rows in (16, 32, 64, 128, 256):
        if not have(lambda f, n, k, m, np_, pf, nt: nt["family"] == 3 and nt["rows"] == rows):
            miss.append(f"skinny {rows} rows")
    for wk in (1, 2, 4, 8):
        if not have(lambda f, n, k, m, np_, pf, nt: nt["family"] == 3 and nt["wk"] == wk):
            miss.append(f"WK {wk}")
    for cpw in (0, 2, 4):
        if not have(lambda f, n, k, m, np_, pf, nt: nt["family"] == 3 and nt["cpw"] == cpw):
            miss.append(f"CPW {cpw}")
    for flag in ("nt", "affine"):
        for v in (0, 1):
            if not have(lambda f, n, k, m, np_, pf, nt: nt["family"] == 3 and nt[flag] == v):
                miss.append(f"{flag} {v}")
    for k in (512, 1024):
        for pair in (0, 1):
            if not have(lambda f, n, kk, m, np_, pf, nt: nt["family"] == 2 and kk == k and nt["pair"] == pair):
                miss.append(f"deep K {k} {'pair' if pair else 'plain'}")
    for form in (1, 3):
        if not have(lambda f, n, k, m, np_, pf, nt: nt["family"] == 4 and nt["wide_form"] == form):
            miss.append(f"wide form {form}")
    for fam in G.FAMILIES:                                       # a ragged last row tile wherever the shape rule allows one (not wide)
        kinds = {nt["family"] for f, n, k, m, np_, pf, nt in notes if f == fam and nt["family"] != 4}
        for kf in kinds:
            if (fam, kf) not in S.ragged:
                miss.append(f"ragged last tile: {fam} on the {G.FAMILY_NAMES[kf]} kernel")
    paths = {G.ln_merge_is_fast(nt, np_) for f, n, k, m, np_, pf, nt in notes if f.startswith("ln_") and nt["family"] != 4}
    if paths != {True, False}:                                   # LdF32LN_T::fast from BM and THREADS of the note and stats_np
        miss.append(f"both LayerNorm merge paths (fast: {sorted(paths)})")
    print(f"{len(notes)} launches, {S.moved} operand elements moved off rounding ties, worst stats_out error {S.stat_worst:.3e}")
    print(f"{'family':14s} {'kernel note':58s} {'n':>4s} {'fp32 maxabs':>12s} {'torch fp32':>11s} {'ratio':>6s} {'bf16 excess':>11s}")
    for (fam, key), (ratio, (err, e32), excess, n) in sorted(S.worst.items()):
        print(f"{fam:14s} {key:58s} {n:4d} {err:12.3e} {e32:11.3e} {ratio:6.2f} {excess:11.3f}")
    if miss:
        pytest.fail("input error: the cases do not reach " + "; ".join(miss))
