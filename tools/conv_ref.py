"""One launch of a face-geometry convolution (hd_conv.hpp, LdConv in hd_gemm.hpp) on its own: inputs whose faces cannot be mistaken for
one another, a plain float64 reference written as a row gather and a matrix product, and the runner that starts the launch through
`hd_debug_conv` (the library's own add_hca / add_down: nothing is forced).  Rounding, guard patterns and bit comparisons are those of
tools/gemm_ref.py.

  * `tap_rows`: for every output pixel the input row of each tap, or the zero row behind the input where the tap leaves the FACE
    (`leak=True`: where it leaves the whole buffer only, i.e. a convolution that takes the neighbouring face for the padding -- what a
    kernel with a wrong border test computes; tests/test_conv_ref_host.py shows that the inputs here tell the two apart);
  * `evaluate`: hca = ReLU(3x3 pad 1 per face + bias), or the centre tap alone on 1 x 1 faces; down = 2x2 stride 2 per face + bias.
    bf16 inputs, bf16-rounded weights, no other rounding: float64, or torch fp32 on the CPU (the reference's own fp32 error, which the
    bounds are measured against);
  * `evaluate_sliced`: the hca sum in fp32 as the staged kernel groups it -- KS slices of the input channels, every slice over all nine
    taps, the partial sums added to the bias in slice order (hd_conv.hpp) -- written from the kernel's description, not from its code;
  * `make_input`: every face its own scale and its own sign per channel, no zero anywhere (border pixels included);
  * `ConvRunner`: one context (created, not finalized), one weight pair per (kind, C) loaded on first use, the input copied per launch
    with NaN-pattern rows behind M, outputs with NaN-pattern guard rows.
Faces are independent, so the reference of a (kind, C, side) is evaluated once at its largest face count and sliced.
(Test infrastructure; tests/test_conv_edges.py, tests/test_conv_ref_host.py.)
"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gemm_ref import GUARD_ROWS, NAN16, NAN32, round_bf16, same_bits, untouched  # noqa: E402,F401

KINDS = {"hca": 0, "down": 1}                                    # include/hifidiff_hip.h HD_CONV_*
# add_hca's table: (C, side) -> (BM, KS, NT, strip) of the ConvCfg that is staged in LDS (hd_conv.hpp); every other pair is gathered
STAGED = {(128, 16): (256, 2, 1, 0), (256, 8): (128, 4, 1, 0), (512, 4): (64, 8, 1, 0), (1024, 2): (32, 8, 1, 0), (256, 16): (256, 2, 2, 0),
          (512, 8): (64, 8, 1, 0), (1024, 4): (64, 8, 2, 0), (2048, 2): (32, 8, 2, 0), (128, 32): (256, 2, 4, 1)}
PIXEL_CLASSES = ("corner", "edge", "interior")


def faces_per_workgroup(C, side):
    bm, _, _, strip = STAGED[(C, side)]
    return 1 if strip or bm <= side * side else bm // (side * side)


# ---------------------------------------------------------------------------------------------- geometry
def tap_rows(faces, side, k, stride, pad, leak=False):
    """[faces * so * so][k * k] input rows (tap-major ky, kx) of a k x k conv on faces of side x side pixels stored row-major, face after
    face; faces * side * side (the zero row) where the tap is padding.  leak: the face border is ignored -- the tap is taken at its
    linear distance dy * side + dx in the buffer and only the ends of the buffer are padding."""
    so = (side + 2 * pad - k) // stride + 1
    f, oy, ox = torch.meshgrid(torch.arange(faces), torch.arange(so), torch.arange(so), indexing="ij")
    f, oy, ox = f.reshape(-1), oy.reshape(-1), ox.reshape(-1)
    M = faces * side * side
    cols = []
    for ky in range(k):
        for kx in range(k):
            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
            lin = (f * side + iy) * side + ix
            inside = (lin >= 0) & (lin < M) if leak else (iy >= 0) & (iy < side) & (ix >= 0) & (ix < side)
            cols.append(torch.where(inside, lin, torch.full_like(lin, M)))
    return torch.stack(cols, 1)


def pixel_class(side):
    """[side * side] 0 corner, 1 edge, 2 interior (a 1 x 1 or 2 x 2 face has corners only)."""
    y, x = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
    by, bx = (y == 0) | (y == side - 1), (x == 0) | (x == side - 1)
    return torch.where(by & bx, 0, torch.where(by | bx, 1, 2)).reshape(-1)


def gather(x, idx):
    """x [M][C], idx [Mo][T] -> [Mo][T * C] (k = tap * C + c), the zero row appended behind x."""
    xz = torch.cat((x, torch.zeros(1, x.shape[1], dtype=x.dtype)))
    return xz[idx].reshape(idx.shape[0], -1)


def weight_matrix(w, centre=False):
    """[N][C][kh][kw] -> [N][kh * kw * C] in the gather's k order; centre: the middle tap alone [N][C]."""
    if centre:
        return w[:, :, w.shape[2] // 2, w.shape[3] // 2].contiguous()
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


# ---------------------------------------------------------------------------------------------- the reference
def weight_matrices(w):
    """(float64, fp32) weight_matrix of the bf16-rounded weight: what `evaluate(wm=...)` takes, so that the tests of several sides of one
    C convert a large weight once.  (The weight goes through torch's own bf16: the same grid as round_bf16, held against it bit for
    bit by the host tests, and quick on 38 M elements.)"""
    m = weight_matrix(w.bfloat16().float())
    return m.double(), m


def evaluate(kind, x, w, b, side, dtype=torch.float64, rounded=True, leak=False, wm=None):
    """x [faces * side^2][C] -> the unrounded value of `out`: hca [M][C], down [M / 4][2 C].  wm: weight_matrix of the weight, rounded
    and in `dtype` already (w is then not read)."""
    if wm is None:
        wm = weight_matrix((w.bfloat16() if rounded else w).to(dtype))
    x, b = (round_bf16(x) if rounded else x).to(dtype), b.to(dtype)
    faces = x.shape[0] // (side * side)
    if kind == "hca":
        if side == 1 and not leak:                               # only the centre tap (index 4 of 9) sees data
            return torch.relu(x @ wm.reshape(wm.shape[0], 9, -1)[:, 4].t() + b)
        return torch.relu(gather(x, tap_rows(faces, side, 3, 1, 1, leak)) @ wm.t() + b)
    return gather(x, tap_rows(faces, side, 2, 2, 0, leak)) @ wm.t() + b


def evaluate_sliced(x, w, b, side, ks, dtype=torch.float32, wm=None):
    """hca in `dtype` with the sum over K = 9 C grouped as the staged kernel groups it: slice s of ks covers channels [s C / ks,
    (s + 1) C / ks) of all nine taps; v = bias, then v += partial_s for s = 0 .. ks - 1, then ReLU."""
    if wm is None:
        wm = weight_matrix(w.bfloat16().to(dtype))
    x, b = round_bf16(x).to(dtype), b.to(dtype)
    faces, C = x.shape[0] // (side * side), x.shape[1]
    a = gather(x, tap_rows(faces, side, 3, 1, 1)).reshape(x.shape[0], 9, C)
    wm = wm.reshape(wm.shape[0], 9, C)
    v = b.expand(x.shape[0], -1).clone()
    for s in range(ks):
        sl = slice(s * C // ks, (s + 1) * C // ks)
        v = v + a[:, :, sl].reshape(x.shape[0], -1) @ wm[:, :, sl].reshape(wm.shape[0], -1).t()
    return torch.relu(v)


# ---------------------------------------------------------------------------------------------- operands
def make_input(faces, side, C, seed=0):
    """bf16 values in an fp32 tensor [faces * side^2][C].  Face f: magnitudes |N(0, 1)| >= 2^-6 times a scale of its own (0.5, 1, 2 in
    turn, times 1 + 0.03 f), and one sign per (face, channel) for all its pixels -- what leaks in from a neighbouring face adds up
    coherently with that face's signs instead of averaging out."""
    gen = torch.Generator().manual_seed(7919 * seed + 104729 * C + side)
    mag = torch.randn(faces, side * side, C, generator=gen).abs().clamp_min(2.0 ** -6)
    scale = torch.tensor([(0.5, 1.0, 2.0)[f % 3] * (1 + 0.03 * f) for f in range(faces)])[:, None, None]
    sign = torch.where(torch.rand(faces, 1, C, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * scale * sign).reshape(faces * side * side, C).bfloat16().float()


def make_weight(kind, C, seed=1234):
    """(w, b): hca [C][C][3][3], down [2 C][C][2][2], variance 1 / K, already on the bf16 grid (the packer's rounding is then exact)."""
    gen = torch.Generator().manual_seed(seed + 31 * C + KINDS[kind])
    n, k = (C, 3) if kind == "hca" else (2 * C, 2)
    w = (torch.randn(n, C, k, k, generator=gen) / (C * k * k) ** 0.5).bfloat16().float()
    return w, torch.randn(n, generator=gen) * 0.5


# ---------------------------------------------------------------------------------------------- the runner
def note_key(kind, note):
    if note["form"] == 1:
        return (f"staged C {note['C']} side {note['side']} BM {note['bm']} KS {note['ks']} NT {note['nt']}{' strip' if note['strip'] else ''}"
                f"{' remap' if note['remap'] else ''}")
    g = note["gemm"]
    return (f"{'centre' if note['centre_only'] else kind} gather {g['rows']} rows WK {g['wk']} CPW {g['cpw']}{' NT' if g['nt'] else ''}"
            f"{' hint %d' % note['hint'] if note['hint'] >= 0 else ''}")


class ConvRunner:
    """A context for hd_debug_conv with one random weight pair per (kind, C), and what the launches of a module noted."""

    def __init__(self):
        from hifidiff_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.ctx = ctypes.c_void_p()
        _lib.check(self.L.hd_create(ctypes.byref(self.ctx), 16, 0))
        self.W = {}
        self.notes = []                                          # (kind, C, side, faces, note dict) of every launch

    def close(self):
        if self.ctx:
            self.L.hd_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def load(self, name, w, b):
        _lib = self._lib
        descs = []
        for suffix, t in ((".weight", w), (".bias", b)):
            if t is None:
                continue
            d = _lib.TensorDesc()
            d.name, d.data, d.ndim, d.is_device = (name + suffix).encode(), t.data_ptr(), t.dim(), 0
            for i, s in enumerate(t.shape):
                d.shape[i] = s
            descs.append(d)
        arr = (_lib.TensorDesc * len(descs))(*descs)
        _lib.check(self.L.hd_load_weights(self.ctx, arr, len(descs)), self.ctx)

    def weight(self, kind, C):
        if (kind, C) not in self.W:
            w, b = make_weight(kind, C)
            self.load(f"{kind}{C}", w, b)
            self.W[(kind, C)] = (w, b)
        return self.W[(kind, C)]

    @staticmethod
    def _guarded(rows, ld, bf16):
        n = (rows + GUARD_ROWS) * ld
        t = torch.empty(n, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        t.view(torch.int16 if bf16 else torch.int32).fill_(NAN16 if bf16 else NAN32)
        return t

    def launch(self, kind, x, C, side, want=("out16", "stats_out"), dry=False, edit=None, name=None):
        """One launch on the rows of x (CPU, bf16 values).  Returns (rc, note dict, {name: CPU tensor [rows + GUARD_ROWS][ld]})."""
        _lib = self._lib
        M = x.shape[0]
        if name is None:
            self.weight(kind, C)
        xd = self._guarded(M, C, True)                           # rows behind M: the NaN pattern
        xd[:M * C] = x.bfloat16().reshape(-1).cuda()
        n, rows = (C, M) if kind == "hca" else (2 * C, M // 4)
        outs = {"out": self._guarded(rows, n, False)}
        d = _lib.ConvDesc()
        d.M, d.C, d.side, d.X, d.out = M, C, side, xd.data_ptr(), outs["out"].data_ptr()
        if "out16" in want:
            outs["out16"] = self._guarded(rows, n, True)
            d.out16 = outs["out16"].data_ptr()
        if "stats_out" in want and kind == "down":
            outs["stats_out"] = self._guarded(rows, 2 * (n // 32), False)
            d.stats_out = outs["stats_out"].data_ptr()
        if edit is not None:
            edit(d)
        note = _lib.ConvNote()
        torch.cuda.synchronize()
        rc = self.L.hd_debug_conv(self.ctx, KINDS[kind], (name or f"{kind}{C}").encode(), None, ctypes.byref(d), _lib.GEMM_DRY_RUN if dry else 0,
                                  ctypes.byref(note), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        nd = {f: getattr(note, f) for f, _ in _lib.ConvNote._fields_ if f != "gemm"}
        nd["gemm"] = {f: getattr(note.gemm, f) for f, _ in _lib.GemmNote._fields_}
        nd["mode"] = ((note.gemm.op_info >> 16) & 0xff) - 1
        if rc == 0 and not dry:
            self.notes.append((kind, C, side, M // (side * side), nd))
        res = {k: t.cpu().reshape(rows + GUARD_ROWS, -1) for k, t in outs.items()}
        res["_x"] = xd.cpu().reshape(M + GUARD_ROWS, C)
        return rc, nd, res

    def error(self):
        m = self.L.hd_last_error(self.ctx)
        return m.decode() if m else ""


# ---------------------------------------------------------------------------------------------- conv1 -> depthwise 3x3 -> gate -> pool
FILM_OFF = 64                                                    # not at the start of the row


def make_dw_operands(C, side, faces, stats_np, per_face=False, face0=0, seed=0, exact=False):
    """The inputs of one HD_CONV_DWGATE launch in the vocabulary of gemm_ref (`a_operand`, `settle_ln` read them): the fp32 residual stream
    X [faces * side^2][C] with a scale per face and a quarter of the rows offset to |mean| / std ~ 40, its bf16 copy "A", its (mean, M2)
    partials in stats_np parts, and FiLM rows (one, or one per face from face0 on) with the bias at FILM_OFF and the gain at FILM_OFF + C.
    The bf16 copy is moved off rounding ties by settle_ln.  exact: nothing rounded, partials float64 (the host test)."""
    import gemm_ref as G
    gen = torch.Generator().manual_seed(15485863 * seed + 104729 * C + 31 * side + stats_np)
    hw = side * side
    M = faces * hw
    scale = torch.tensor([(0.5, 1.0, 2.0)[f % 3] * (1 + 0.03 * f) for f in range(faces)]).repeat_interleave(hw)[:, None]
    std = scale * (0.5 + torch.rand(M, 1, generator=gen))
    off = torch.where(torch.arange(M)[:, None] % 4 == 3, 40.0 * std, torch.randn(M, 1, generator=gen) * std)
    X = torch.randn(M, C, generator=gen) * std + off
    cnt = C // stats_np
    t = X.double().reshape(M, stats_np, cnt)
    mean = t.mean(-1)
    stats = torch.stack((mean, (t - mean[..., None]).pow(2).sum(-1)), -1)
    nrows = face0 + faces if per_face else 1
    film = torch.zeros(nrows, FILM_OFF + 2 * C + 32)
    gsign = torch.where(torch.rand(nrows, C, generator=gen) < 0.5, -1.0, 1.0)
    film[:, FILM_OFF + C:FILM_OFF + 2 * C] = gsign * (0.25 + torch.randn(nrows, C, generator=gen).abs() * 0.75)
    film[:, FILM_OFF:FILM_OFF + C] = torch.randn(nrows, C, generator=gen) * 0.5
    ops = {"family": "ln_gate", "M": M, "hw": hw, "side": side, "C": C, "faces": faces, "face0": face0, "per_face": per_face, "film": film,
           "gain_off": FILM_OFF + C, "bias_off": FILM_OFF, "stats_np": stats_np, "stats_cnt": cnt,
           "A": X.double() if exact else X.bfloat16().float(), "stats_in": stats if exact else stats.float()}
    ops["moved"] = 0 if exact else G.settle_ln(ops)
    return ops


def make_dw_weights(C, seed=4321):
    """conv1 [2C][C] on the bf16 grid + bias, conv2 [2C][1][3][3] fp32 (taps ~ N(0, 1/3): nine of them keep the scale) + bias."""
    gen = torch.Generator().manual_seed(seed + 17 * C)
    w1 = (torch.randn(2 * C, C, generator=gen) / C ** 0.5).bfloat16().float()
    return w1, torch.randn(2 * C, generator=gen) * 0.5, torch.randn(2 * C, 1, 3, 3, generator=gen) / 3.0, torch.randn(2 * C, generator=gen) * 0.5


def depthwise_gate(t1, w2, b2, faces, side):
    """t1 [M][2C] -> (g [M][C], pooled [faces][C]): u = b2 + the nine taps of the 3x3 pad-1 depthwise conv per face, g = u[:C] * u[C:]
    unrounded, pooled = the face mean of g.  In the dtype of t1."""
    C2 = t1.shape[1]
    idx = tap_rows(faces, side, 3, 1, 1)
    tz = torch.cat((t1, torch.zeros(1, C2, dtype=t1.dtype)))
    w = w2.to(t1.dtype).reshape(C2, 9)
    u = b2.to(t1.dtype).expand(t1.shape[0], -1).clone()
    for t in range(9):
        u += w[:, t] * tz[idx[:, t]]
    g = u[:, :C2 // 2] * u[:, C2 // 2:]
    return g, g.reshape(faces, side * side, -1).mean(1)


def evaluate_dw(ops, w1, b1, w2, b2, dtype=torch.float64, rounded=True):
    """{"t1": conv1 + bias of the LayerNorm + FiLM rows (rounded to bf16 where the loader rounds them), "g", "pooled"} unrounded."""
    import gemm_ref as G
    a = G.a_operand(ops, dtype, rounded)
    t1 = a @ (w1.bfloat16() if rounded else w1).to(dtype).t() + b1.to(dtype)
    g, pooled = depthwise_gate(t1, w2, b2, ops["faces"], ops["side"])
    return {"t1": t1, "g": g, "pooled": pooled}


def dw_slice(ops, faces):
    """The first `faces` faces of an operand set."""
    M = faces * ops["hw"]
    return dict(ops, M=M, faces=faces, A=ops["A"][:M], stats_in=ops["stats_in"][:M])


def dw_note_key(ops, note):
    g = note["gemm"]
    path = {1: "fused", 2: "strip", 3: "unfused"}[note["dw_path"]]
    if note["dw_path"] == 2:
        return f"strip C {ops['C']} side {ops['side']}"
    fam = {1: "tall", 2: "deep", 3: "skinny", 4: "wide"}.get(g["family"], "?")
    return (f"{path} hw {ops['hw']}{' per-face' if ops['per_face'] else ''} {fam} {g['rows']} rows WK {g['wk']}"
            f"{' form %d' % g['wide_form'] if g['wide_form'] else ''}")


class DwRunner(ConvRunner):
    """hd_debug_conv(HD_CONV_DWGATE) on the context of a ConvRunner: one weight set dw<C> / dwc<C> per C."""

    def dw_weight(self, C):
        if ("dw", C) not in self.W:
            w1, b1, w2, b2 = make_dw_weights(C)
            self.load(f"dw{C}", w1, b1)
            self.load(f"dwc{C}", w2, b2)
            self.W[("dw", C)] = (w1, b1, w2, b2)
        return self.W[("dw", C)]

    def launch_dw(self, ops, dry=False, edit=None, names=None):
        """One launch.  Returns (rc, note dict, {"G", "pooled", "pooled16", "T1"}: CPU tensors with GUARD_ROWS guard rows; T1 as
        [2 M + bands + GUARD_ROWS][C] rows of C floats)."""
        _lib = self._lib
        C, side, M, faces = ops["C"], ops["side"], ops["M"], ops["faces"]
        if names is None:
            self.dw_weight(C)
        xd = self._guarded(M, C, True)
        xd[:M * C] = ops["A"].bfloat16().reshape(-1).cuda()
        np_ = ops["stats_np"]
        sd = self._guarded(M, 2 * np_, False)
        sd[:M * 2 * np_] = ops["stats_in"].float().reshape(-1).cuda()
        film = ops["film"].float().contiguous().cuda()
        t1_rows = 2 * M + faces * ((side + 7) // 8)
        outs = {"G": self._guarded(M, C, True), "pooled": self._guarded(faces, C, False), "pooled16": self._guarded(faces, C, True),
                "T1": self._guarded(t1_rows, C, False)}
        d = _lib.ConvDesc()
        d.M, d.C, d.side, d.face0, d.stats_np, d.stats_cnt = M, C, side, ops["face0"], np_, ops["stats_cnt"]
        d.film_off, d.film_face_stride, d.T1_elems = ops["bias_off"], (film.shape[1] if ops["per_face"] else 0), t1_rows * C
        d.X, d.stats_in, d.film = xd.data_ptr(), sd.data_ptr(), film.data_ptr()
        d.G, d.pooled, d.pooled16, d.T1 = outs["G"].data_ptr(), outs["pooled"].data_ptr(), outs["pooled16"].data_ptr(), outs["T1"].data_ptr()
        if edit is not None:
            edit(d)
        note = _lib.ConvNote()
        n1, n2 = names or (f"dw{C}", f"dwc{C}")
        torch.cuda.synchronize()
        rc = self.L.hd_debug_conv(self.ctx, 2, n1.encode(), None if n2 is None else n2.encode(), ctypes.byref(d), _lib.GEMM_DRY_RUN if dry else 0,
                                  ctypes.byref(note), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        nd = {f: getattr(note, f) for f, _ in _lib.ConvNote._fields_ if f != "gemm"}
        nd["gemm"] = {f: getattr(note.gemm, f) for f, _ in _lib.GemmNote._fields_}
        if rc == 0 and not dry:
            self.notes.append(("dw", C, side, faces, dict(nd, per_face=ops["per_face"], stats_np=np_)))
        rows = {"G": M, "pooled": faces, "pooled16": faces, "T1": t1_rows}
        res = {k: t.cpu().reshape(rows[k] + GUARD_ROWS, C) for k, t in outs.items()}
        res["_x"], res["_stats"] = xd.cpu().reshape(M + GUARD_ROWS, C), sd.cpu().reshape(M + GUARD_ROWS, 2 * np_)
        return rc, nd, res
