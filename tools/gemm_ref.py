"""One launch of the shared GEMM kernels (hd_gemm.hpp, hd_wide.hpp) on its own: random operands of a (family, N, K), a float64
reference with the kernels' rounding points and no others, and the runner that starts the launch through `hd_debug_gemm` (the library's
own add_gemm: nothing is forced) and holds what it wrote against the reference.

  * `round_bf16`: round to nearest even onto the bf16 grid, in float64 arithmetic (no bit tricks shared with a kernel);
  * `evaluate`: per family the loader's transform (F32: x * a_scale; BF16S: bf16(x) * rowscale[row / hw]; LN: fma(fma(bf16(x), rstd,
    -mean * rstd), gain, bias) with (mean, rstd) merged from the (mean, M2) partials handed in, ln_eps inside the root) rounded to
    bf16, the bf16 weight, the accumulation, and the epilogue structs of hd_gemm.hpp (BIASF32, RESID with its gated bf16 output, GATE,
    PIXSHUF, BIASBF16) -- in float64, or in torch fp32 on the CPU when asked: the reference's own fp32 error, which the bounds are
    measured against.  `rounded=False` drops every bf16 rounding (tests/test_gemm_ref_host.py holds that form against torch);
  * `make_operands`, `settle_ln`: the operands of a case.  A quarter of the LayerNorm rows is offset (|row mean| / row std ~ 40).
    The bf16 copy a LayerNorm loader normalises is moved by whole bf16 steps where the transformed value would land so close to a bf16
    rounding tie that two correct fp32 evaluations could round it differently: the A operand of every evaluation is then the same,
    and the fp32 bound measures the accumulation and the epilogue, not where a coin fell;
  * `Runner`: one context (created, not finalized), weights loaded once, outputs with guard rows prefilled with a NaN pattern.
Rows are independent, so the reference of an operand set is evaluated once at its largest M and sliced.
(Test infrastructure; tests/test_gemm_edges.py, tests/test_gemm_ref_host.py.)
"""
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LK = {"F32": 0, "LN": 1, "BF16": 2, "BF16S": 3}                  # hd_dispatch.hpp LdKind / EpKind
EK = {"BIASF32": 0, "RESID": 1, "GATE": 2, "PIXSHUF": 3, "BIASBF16": 4}
FAMILIES = {"f32_biasf32": ("F32", "BIASF32"), "f32_pixshuf": ("F32", "PIXSHUF"), "bf16_resid": ("BF16", "RESID"), "bf16s_resid": ("BF16S", "RESID"),
            "bf16_biasbf16": ("BF16", "BIASBF16"), "bf16_pixshuf": ("BF16", "PIXSHUF"), "bf16_biasf32": ("BF16", "BIASF32"),
            "ln_gate": ("LN", "GATE"), "ln_biasf32": ("LN", "BIASF32")}
BF16_OUT = ("GATE", "BIASBF16")                                  # epilogues whose `out` is bf16
LN_EPS = 1e-6
BF16_MAX = float.fromhex("0x1.fep127")
GUARD_ROWS = 64
NAN32, NAN16 = 0x7FC12345, 0x7FC5                                 # non-canonical quiet NaNs: nothing computes these bits


# ---------------------------------------------------------------------------------------------- bf16 grid
def _exp2(e):
    return torch.ldexp(torch.ones(e.shape, dtype=torch.float64), e)


def bf16_ulp(x):
    """Spacing of the bf16 grid in the binade of |x| (float64; denormals: 2^-133)."""
    _, e = torch.frexp(x.double())
    return _exp2((e - 1).clamp(min=-126) - 7)


def round_bf16(x):
    """x (float32 or float64) rounded to the nearest bf16 value, ties to even, in x's dtype."""
    x64 = x.double()
    ulp = bf16_ulp(x64)
    r = torch.round(x64 / ulp) * ulp                            # torch.round: half to even; the scaling is exact
    r = torch.where(r.abs() > BF16_MAX, torch.copysign(torch.full_like(r, float("inf")), x64), r)
    return r.to(x.dtype)


def tie_distance(y):
    """Distance of y (float64) to the nearest midpoint between two bf16 values."""
    ulp = bf16_ulp(y)
    t = y / ulp
    return ((t - torch.floor(t)) - 0.5).abs() * ulp


# ---------------------------------------------------------------------------------------------- the reference
def merge_partials(stats, cnt, dtype=torch.float64):
    """stats [M][np][2] (mean, M2) partials of cnt elements each -> (mean, rstd) of the row, biased variance, LN_EPS inside the root."""
    s = stats.to(dtype)
    mean = s[..., 0].sum(1) / s.shape[1]
    d = s[..., 0] - mean[:, None]
    m2 = (s[..., 1] + cnt * d * d).sum(1)
    return mean, 1.0 / torch.sqrt(m2 / (cnt * s.shape[1]) + LN_EPS)


def _fma(a, b, c):
    """a * b + c with one rounding in the dtype of a (float32: evaluated in float64, where the product is exact)."""
    if a.dtype == torch.float64:
        return a * b + c
    return (a.double() * b.double() + c.double()).to(a.dtype)


def _act(v, act):
    return torch.relu(v) if act == 1 else 1.0 / (1.0 + torch.exp(-v)) if act == 2 else v


def shuffle_rows(y, win):
    """[M][4 C] in the weight's own column order n = 4 c + 2 i + j -> [4 M][C]: row ((b * 2 Win + 2 h + i) * 2 Win + 2 w + j)."""
    M, N = y.shape
    return y.reshape(M // (win * win), win, win, N // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(4 * M, N // 4)


def a_operand(ops, dtype=torch.float64, rounded=True):
    """The A operand as the MFMA sees it: the loader's transform, then bf16."""
    lk = FAMILIES[ops["family"]][0]
    q = (lambda x: x) if not rounded else round_bf16 if dtype == torch.float64 else (lambda x: x.bfloat16().to(dtype))
    x = ops["A"].to(dtype)
    M = x.shape[0]
    face = torch.arange(M) // ops.get("hw", 1)
    if lk == "F32":
        return q(x * ops["a_scale"])
    if lk == "BF16":
        return q(x)
    if lk == "BF16S":
        return q(q(x) * ops["rowscale"].to(dtype)[face])
    mean, rstd = merge_partials(ops["stats_in"], ops["stats_cnt"], dtype)
    K, film = x.shape[1], ops["film"].to(dtype)
    rows = ops["face0"] + face if ops["per_face"] else torch.zeros(M, dtype=torch.long)
    gain, bias = film[rows, ops["gain_off"]:ops["gain_off"] + K], film[rows, ops["bias_off"]:ops["bias_off"] + K]
    mu = -mean * rstd
    return q(_fma(_fma(q(x), rstd[:, None], mu[:, None]), gain, bias))


def evaluate(ops, dtype=torch.float64, rounded=True):
    """{"v": the unrounded epilogue value in the layout of `out`, "g": the unrounded gated value of RESID's outg16 (or None)}."""
    ek = FAMILIES[ops["family"]][1]
    q = (lambda x: x) if not rounded else round_bf16 if dtype == torch.float64 else (lambda x: x.bfloat16().to(dtype))
    a = a_operand(ops, dtype, rounded)
    M = a.shape[0]
    acc = a @ q(ops["W"].to(dtype)).t()
    bias = ops["bias"].to(dtype) if ops.get("bias") is not None else torch.zeros(acc.shape[1], dtype=dtype)
    g = None
    if ek == "BIASF32":
        v = _act(acc + bias, ops.get("act", 0))
    elif ek == "RESID":
        v = _fma(acc + bias, ops["rscale"].to(dtype), ops["resid"].to(dtype))
        if ops.get("gate_c") is not None:
            face = torch.arange(M) // ops["hw"]
            add = ops["add_src"].to(dtype) if ops.get("add_src") is not None else 0.0
            g = (v + add) * ((1.0 + ops["gate_c"].to(dtype)[face]) + ops["gate_s"].to(dtype)[:, None])
    elif ek == "GATE":
        h = acc.shape[1] // 2
        v = (acc[:, :h] + bias[:h]) * (acc[:, h:] + bias[h:])
    elif ek == "PIXSHUF":                                       # no bias (add_up); the skip is laid out like the output
        v = shuffle_rows(acc, ops["Win"]) if ops.get("shuffle_r", 1) == 2 else acc
        if ops.get("resid") is not None:
            v = v + ops["resid"].to(dtype)
    else:                                                       # BIASBF16
        v = acc + bias
        if ops.get("resid") is not None:
            v = v + q(ops["resid"].to(dtype))
        v = _act(v, ops.get("act", 0))
    return {"v": v, "g": g}


def tile_stats(v):
    """(mean, M2) per row and 32-column tile of v, float64: [M][N / 32][2]."""
    t = v.double().reshape(v.shape[0], -1, 32)
    mean = t.mean(-1)
    return torch.stack((mean, (t - mean[..., None]).pow(2).sum(-1)), -1)


# ---------------------------------------------------------------------------------------------- operands
def settle_ln(ops, max_iter=64):
    """Moves elements of the bf16 copy ops["A"] up by bf16 steps until no transformed value lies within the reach of an fp32
    evaluation's error of a bf16 rounding tie: |y - tie| > 2^-19 ((|x rstd| + |mean rstd|) |gain| + |y|), which covers the rounding of
    -mean * rstd, an ulp or two of difference in mean and rstd between two merge orders, and the two fused multiply-adds.  Returns the
    number of elements moved; raises ValueError when an element cannot be settled."""
    mean, rstd = merge_partials(ops["stats_in"], ops["stats_cnt"])
    x = ops["A"].double()
    M, K = x.shape
    face = torch.arange(M) // ops.get("hw", 1)
    rows = ops["face0"] + face if ops["per_face"] else torch.zeros(M, dtype=torch.long)
    film = ops["film"].double()
    gain, bias = film[rows, ops["gain_off"]:ops["gain_off"] + K], film[rows, ops["bias_off"]:ops["bias_off"] + K]
    mu, rs = (-mean * rstd)[:, None], rstd[:, None]
    moved = torch.zeros_like(x, dtype=torch.bool)
    for _ in range(max_iter):
        y = (x * rs + mu) * gain + bias
        bad = tie_distance(y) <= 2.0 ** -19 * (((x * rs).abs() + mu.abs()) * gain.abs() + y.abs())
        if not bool(bad.any()):
            ops["A"] = x.to(torch.float32)
            return int(moved.sum())
        moved |= bad
        x = torch.where(bad, round_bf16(x + torch.maximum(bf16_ulp(x), bf16_ulp(1.0 / rs))), x)      # a bf16 step of x, at least one at the row's std
    raise ValueError(f"{int(bad.sum())} LayerNorm elements stay within reach of a bf16 rounding tie")


def settle_scaled(ops, max_iter=64):
    """The same for the two loaders that multiply once in fp32 before they round (F32: x * a_scale, BF16S: bf16(x) * rowscale): a product
    within 2^-22 |y| of a tie would round differently in fp32 and in float64, identically in every fp32 evaluation -- an error the fp32
    bound would then allow every kernel.  F32 rows are fp32 (moved by 2^-12 x), BF16S rows bf16 (moved by a bf16 step)."""
    f32 = FAMILIES[ops["family"]][0] == "F32"
    x = ops["A"].double()
    scale = ops["a_scale"] if f32 else ops["rowscale"].double()[torch.arange(x.shape[0]) // ops["hw"]]
    moved = torch.zeros_like(x, dtype=torch.bool)
    for _ in range(max_iter):
        y = x * scale
        bad = tie_distance(y) <= 2.0 ** -22 * y.abs()
        if not bool(bad.any()):
            ops["A"] = x.to(torch.float32)
            return int(moved.sum())
        moved |= bad
        x = torch.where(bad, (x * (1 + 2.0 ** -12)).float().double() if f32 else round_bf16(x + bf16_ulp(x)), x)
    raise ValueError(f"{int(bad.sum())} scaled elements stay within reach of a bf16 rounding tie")


def make_operands(family, N, K, M, hw=1, seed=0, per_face=False, stats_np=1, face0=0, shuffle_r=1, win=4, gated=False, act=0, ldo_pad=0, exact=False):
    """Random operands of one (family, N, K) at M rows, CPU tensors.  bf16 operands are fp32 tensors holding bf16 values.  W and bias
    are NOT part of it: they come from the runner's weight set (one per (N, K)).  exact: nothing is rounded to bf16 and the partials stay
    float64 (the operands of `evaluate(rounded=False)`, tests/test_gemm_ref_host.py)."""
    lk, ek = FAMILIES[family]
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 31 * K + len(family))
    rn = lambda *s: torch.randn(*s, generator=gen)                # noqa: E731
    ops = {"family": family, "M": M, "hw": hw, "face0": face0, "per_face": per_face, "act": act, "shuffle_r": shuffle_r, "Win": win}
    faces = M // hw if M % hw == 0 else None
    if lk == "F32":
        ops["A"], ops["a_scale"] = rn(M, K), 0.75
    elif lk in ("BF16", "BF16S"):
        ops["A"] = rn(M, K) if exact else rn(M, K).bfloat16().float()
        if lk == "BF16S":
            ops["rowscale"] = 0.25 + torch.rand(faces, K, generator=gen)
    else:
        std = 0.5 + 1.5 * torch.rand(M, 1, generator=gen)
        off = torch.where(torch.arange(M)[:, None] % 4 == 3, 40.0 * std, rn(M, 1) * std)      # a quarter of the rows: |mean| / std ~ 40
        X = rn(M, K) * std + off                                 # the fp32 residual stream: the partials describe these values,
        ops["A"] = X.double() if exact else X.bfloat16().float()      # the loader normalises their bf16 copy
        cnt = K // stats_np
        t = X.double().reshape(M, stats_np, cnt)
        mean = t.mean(-1)
        ops["stats_in"] = torch.stack((mean, (t - mean[..., None]).pow(2).sum(-1)), -1)
        if not exact:
            ops["stats_in"] = ops["stats_in"].float()
        ops["stats_np"], ops["stats_cnt"] = stats_np, cnt
        ops["ratio"] = (X.double().mean(1).abs() / X.double().std(1, unbiased=False))
        nrows = face0 + faces if per_face else 1
        ops["bias_off"], ops["gain_off"] = 64, 64 + K + 32       # not at the start of the row, not adjacent
        film = torch.zeros(nrows, 64 + 2 * K + 96)
        gsign = torch.where(torch.rand(nrows, K, generator=gen) < 0.5, -1.0, 1.0)
        film[:, ops["gain_off"]:ops["gain_off"] + K] = gsign * (0.25 + rn(nrows, K).abs() * 0.75)
        film[:, ops["bias_off"]:ops["bias_off"] + K] = rn(nrows, K) * 0.5
        ops["film"] = film
        ops["moved"] = 0 if exact else settle_ln(ops)
    if lk in ("F32", "BF16S") and not exact:
        ops["moved"] = settle_scaled(ops)
    ncols = N // 2 if ek == "GATE" else N // 4 if shuffle_r == 2 else N
    rows_out = 4 * M if shuffle_r == 2 else M
    ops["ldo"] = ncols + ldo_pad
    if ek == "RESID":
        ops["resid"], ops["rscale"] = rn(M, N), rn(N) * 0.5
        if gated:
            ops["gate_c"], ops["gate_s"], ops["add_src"] = torch.rand(faces, N, generator=gen) * 0.5, torch.rand(M, generator=gen) * 0.5, rn(M, N)
    elif ek == "PIXSHUF":
        ops["resid"] = rn(rows_out, ncols)
    elif ek == "BIASBF16":
        ops["resid"] = rn(M, N) if exact else rn(M, N).bfloat16().float()
    return ops


def slice_rows(ops, M):
    """The first M rows of an operand set (faces: the first M / hw)."""
    out = dict(ops, M=M)
    hw, r = ops["hw"], 4 if ops["shuffle_r"] == 2 else 1
    for k in ("A", "stats_in", "gate_s", "add_src"):
        if ops.get(k) is not None:
            out[k] = ops[k][:M]
    if ops.get("resid") is not None:
        out["resid"] = ops["resid"][:M * r]
    for k in ("rowscale", "gate_c"):
        if ops.get(k) is not None:
            out[k] = ops[k][:M // hw]
    return out


# ---------------------------------------------------------------------------------------------- the runner
FAMILY_NAMES = {1: "tall", 2: "deep", 3: "skinny", 4: "wide"}


def note_key(note):
    return (f"{FAMILY_NAMES.get(note['family'], '?')} {note['rows']} rows{' pair' if note['pair'] else ''} WK {note['wk']} CPW {note['cpw']}"
            f"{' NT' if note['nt'] else ''}{' form %d' % note['wide_form'] if note['wide_form'] else ''}{' affine' if note['affine'] else ''}")


def ln_merge_is_fast(note, stats_np):
    """LdF32LN_T::fast for the workgroup the note describes (tall, deep, skinny; the wide kernel has a merge of its own)."""
    bm, th = note["rows"], note["threads"]
    tpr = 16 if th // bm >= 16 else max(th // bm, 1)
    return stats_np <= 4 * tpr and bm * tpr <= th


class Runner:
    """A context for hd_debug_gemm with one random weight pair g<N>x<K> per (N, K), and what the launches of a module noted."""

    def __init__(self, shapes, seed=1234):
        from hifidiff_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.ctx = ctypes.c_void_p()
        _lib.check(self.L.hd_create(ctypes.byref(self.ctx), 16, 0))
        gen = torch.Generator().manual_seed(seed)
        self.W, descs, keep = {}, [], []
        for N, K in sorted(set(shapes)):
            w, b = torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen) * 0.5
            self.W[(N, K)] = (w, b)
            for suffix, t in ((".weight", w), (".bias", b)):
                d = _lib.TensorDesc()
                d.name, d.data, d.ndim, d.is_device = f"g{N}x{K}{suffix}".encode(), t.data_ptr(), t.dim(), 0
                for i, s in enumerate(t.shape):
                    d.shape[i] = s
                descs.append(d)
                keep.append(t)
        arr = (_lib.TensorDesc * len(descs))(*descs)
        _lib.check(self.L.hd_load_weights(self.ctx, arr, len(descs)), self.ctx)
        self.notes = []                                          # (family, N, K, M, stats_np, per_face, note dict) of every launch
        self.dev = {}

    def close(self):
        if self.ctx:
            self.L.hd_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def with_weight(self, ops, N, K):
        w, b = self.W[(N, K)]
        return dict(ops, W=w, bias=b, N=N, K=K)

    # -- device side
    def _up(self, ops, key, bf16=False):
        t = ops.get(key)
        if t is None:
            return None
        ck = (id(t), bf16)
        if ck not in self.dev:
            self.dev[ck] = (t, (t.bfloat16() if bf16 else t.float()).contiguous().cuda())      # keeps t alive: ids stay unique
        return self.dev[ck][1]

    @staticmethod
    def _guarded(rows, ld, bf16):
        n = (rows + GUARD_ROWS) * ld
        if bf16:
            t = torch.empty(n, dtype=torch.bfloat16, device="cuda")
            t.view(torch.int16).fill_(NAN16)
        else:
            t = torch.empty(n, dtype=torch.float32, device="cuda")
            t.view(torch.int32).fill_(NAN32)
        return t

    def launch(self, ops, full, want=("out16", "stats_out"), dry=False, edit=None):
        """One launch of the first ops["M"] rows of the operand set `full` (device copies are made once per set).  Returns (rc, note dict,
        {name: CPU tensor [rows + GUARD_ROWS][ld]} of every output asked for).  edit(desc): a last change to the descriptor (refusals)."""
        _lib = self._lib
        lk, ek = FAMILIES[ops["family"]]
        M, N, K, r = ops["M"], ops["N"], ops["K"], ops["shuffle_r"]
        d = _lib.GemmDesc()
        d.M, d.hw, d.face0, d.act, d.shuffle_r, d.Win = M, ops["hw"], ops["face0"], ops["act"], r, ops["Win"]
        d.stats_np, d.stats_cnt, d.a_scale = ops.get("stats_np", 1), ops.get("stats_cnt", 1), ops.get("a_scale", 1.0)
        lda_pad = ops.get("lda_pad", 0)                          # lda != K keeps a shape away from the wide kernel
        d.lda, d.ldo, d.ldr = K + lda_pad, ops["ldo"], (N if ek in ("RESID", "BIASBF16") else 0)
        ptr = lambda t: None if t is None else t.data_ptr()        # noqa: E731
        a_dev = self._up(full, "A", bf16=lk != "F32")
        if lda_pad:
            if ("pad", id(full["A"])) not in self.dev:
                self.dev[("pad", id(full["A"]))] = (full["A"], F.pad(a_dev, (0, lda_pad)).contiguous())
            a_dev = self.dev[("pad", id(full["A"]))][1]
        d.A = ptr(a_dev)
        if lk == "LN":
            d.stats_in, d.film = ptr(self._up(full, "stats_in")), ptr(self._up(full, "film"))
            d.film_gain_off, d.film_bias_off = ops["gain_off"], ops["bias_off"]
            d.film_face_stride = full["film"].shape[1] if ops["per_face"] else 0
        if lk == "BF16S":
            d.rowscale = ptr(self._up(full, "rowscale"))
        rows_out = 4 * M if r == 2 else M
        if ek == "RESID":
            d.resid, d.rscale = ptr(self._up(full, "resid")), ptr(self._up(full, "rscale"))
            if ops.get("gate_c") is not None:
                d.gate_c, d.gate_s, d.add_src = ptr(self._up(full, "gate_c")), ptr(self._up(full, "gate_s")), ptr(self._up(full, "add_src"))
        elif ek == "BIASBF16":
            d.resid = ptr(self._up(full, "resid", bf16=True))
        outs = {"out": self._guarded(rows_out, ops["ldo"], ek in BF16_OUT)}
        if ek == "PIXSHUF":                                     # the skip in the layout of out, with out's leading dimension
            res = torch.zeros(rows_out, ops["ldo"])
            res[:, :full["resid"].shape[1]] = full["resid"][:rows_out]
            outs["_resid"] = res.cuda()
            d.resid = outs["_resid"].data_ptr()
        if ek not in BF16_OUT:
            if "out16" in want:
                outs["out16"] = self._guarded(rows_out, ops["ldo"], True)
                d.out16 = outs["out16"].data_ptr()
            if "stats_out" in want:
                outs["stats_out"] = self._guarded(rows_out, 2 * ((ops["ldo"] if r == 2 else N) // 32), False)
                d.stats_out = outs["stats_out"].data_ptr()
        if ek == "RESID" and ops.get("gate_c") is not None:
            outs["outg16"] = self._guarded(rows_out, ops["ldo"], True)
            d.outg16 = outs["outg16"].data_ptr()
        d.out = outs["out"].data_ptr()
        if edit is not None:
            edit(d)
        note = _lib.GemmNote()
        name = f"g{N}x{K}".encode()
        torch.cuda.synchronize()
        rc = self.L.hd_debug_gemm(self.ctx, name, LK[lk], EK[ek], ctypes.byref(d), _lib.GEMM_DRY_RUN if dry else 0, ctypes.byref(note),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        nd = {f: getattr(note, f) for f, _ in _lib.GemmNote._fields_}
        nd["mode"], nd["affine"], nd["w_nt"] = ((note.op_info >> 16) & 0xff) - 1, (note.op_info >> 24) & 1, (note.op_info >> 25) & 1
        if rc == 0 and not dry:
            self.notes.append((ops["family"], N, K, M, ops.get("stats_np", 0), ops["per_face"], nd))
        res = {}
        for k, t in outs.items():
            if not k.startswith("_"):
                ld = t.numel() // (rows_out + GUARD_ROWS)
                res[k] = t.cpu().reshape(rows_out + GUARD_ROWS, ld)
        return rc, nd, res

    def error(self):
        m = self.L.hd_last_error(self.ctx)
        return m.decode() if m else ""


def untouched(t):
    """Every element of t (fp32 or bf16, CPU) still holds the guard pattern."""
    if t.dtype == torch.bfloat16:
        return bool((t.view(torch.int16) == NAN16).all())
    return bool((t.view(torch.int32) == NAN32).all())


def same_bits(a, b):
    v = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return bool((a.contiguous().view(v) == b.contiguous().view(v)).all())
