// hd_lpips.hip -- LPIPS-AlexNet v0.1 (Zhang et al. 2018) of decoded faces against a reference: the context kind, its strict manifest, its
// per-(batch, side) workspace, its launch program and the entry points hd_lpips_create / hd_lpips.  The contract is in
// include/hifidiff_hip.h; the kernels that are not convolutions are in hd_lpips.hpp.  The `lpips` package and pyiqa are absent: parity
// with them, and the key names below (from memory of the package's full-model state dict), are unpinned.
#include "hd_internal.hpp"
#include "hd_args.hpp"
#include "hd_lpips.hpp"

using namespace hd_args;

namespace {

struct LpConvSpec { const char* name; int cout, cin, k, stride, pad; };
// torchvision AlexNet `features` as the package slices it: the index in the name is the module's position in features
const LpConvSpec kLpConv[LP_LAYERS] = {{"net.slice1.0", 64, 3, 11, 4, 2}, {"net.slice2.3", 192, 64, 5, 1, 2}, {"net.slice3.6", 384, 192, 3, 1, 1},
                                       {"net.slice4.8", 256, 384, 3, 1, 1}, {"net.slice5.10", 256, 256, 3, 1, 1}};
const char* const kLpOpName[LP_LAYERS] = {"slice1.conv", "slice2.conv", "slice3.conv", "slice4.conv", "slice5.conv"};

std::vector<std::pair<std::string, Shape>> build_lpips_manifest() {
    std::vector<std::pair<std::string, Shape>> m;
    for (const auto& s : kLpConv) m_conv(m, s.name, s.cout, s.cin, s.k, s.k);
    for (int k = 0; k < LP_LAYERS; ++k) m.push_back({"lin" + std::to_string(k) + ".model.1.weight", {1, kLpConv[k].cout, 1, 1}});
    return m;
}

// tap sides of an input of side R: s1, s2, s3
void lp_sides(int R, int s[3]) {
    s[0] = (R - 7) / 4 + 1; s[1] = (s[0] - 3) / 2 + 1; s[2] = (s[1] - 3) / 2 + 1;
}

int alloc_lpips_new(hd_ctx* c, Workspace& w, int B, int R) {
    auto& v = w.lws;
    int s[3];
    lp_sides(R, s);
    const size_t n = 2 * (size_t)B, p1 = n * s[0] * s[0], p2 = n * s[1] * s[1], p3 = n * s[2] * s[2];
    int rc = 0;
    rc |= ws_alloc(c, &v.in8, n * R * R);
    rc |= ws_alloc(c, &v.f[0], p1 * 64); rc |= ws_alloc(c, &v.pool[0], p2 * 64);
    rc |= ws_alloc(c, &v.f[1], p2 * 192); rc |= ws_alloc(c, &v.pool[1], p3 * 192);
    rc |= ws_alloc(c, &v.f[2], p3 * 384); rc |= ws_alloc(c, &v.f[3], p3 * 256); rc |= ws_alloc(c, &v.f[4], p3 * 256);
    size_t wgs = 0;
    for (int k = 0; k < LP_LAYERS; ++k) { const int side = s[k < 2 ? k : 2]; wgs += ((size_t)side * side + LP_POS_PER_WG - 1) / LP_POS_PER_WG; }
    rc |= ws_alloc(c, &v.part, (size_t)B * wgs);
    v.B = B; v.R = R;
    w.B = B;
    return rc;
}
// one workspace per (batch, scored side)
int alloc_lpips(hd_ctx* c, int B, int R) {
    return switch_workspace(c, B + 8192 * (R / 8), [&](Workspace& w) { return alloc_lpips_new(c, w, B, R); });
}

// conv (k x k, stride, pad) + bias + ReLU on a channels-last bf16 map of N faces: the im2col loader of the shared GEMM family, as the
// ResNet-50 conv1 runs (hd_lib.hip add_resconv)
void lp_conv(hd_ctx* c, std::vector<Op>& prog, const std::string& name, const PackedW& w, const LpConvSpec& s, const unsigned short* in, int N, int Hin,
             unsigned short* out) {
    const int Hout = (Hin + 2 * s.pad - s.k) / s.stride + 1, cin = w.K / (s.k * s.k);      // cin: as packed (3 -> 8)
    GemmP p = base_gemm(w, N * Hout * Hout);
    p.A = in; p.out = out; p.ldo = s.cout; p.act = 1;
    p.lda = cin; p.Hin = Hin; p.Win = Hin; p.Cin = cin; p.KH = s.k; p.KW = s.k; p.stride = s.stride; p.pad = s.pad;
    p.Hout = Hout; p.Wout = Hout; p.ntaps = s.k * s.k;
    add_gemm(c, prog, name, p, LK_CONV_BF16, EK_BIASBF16);
}

void lp_pool(std::vector<Op>& prog, const std::string& name, const unsigned short* in, unsigned short* out, int N, int H, int C) {
    const int Ho = (H - 3) / 2 + 1;
    const size_t total = (size_t)N * Ho * Ho * (C / 8);
    prog.push_back({name, [=](hipStream_t s) -> hipError_t {
                        hipLaunchKernelGGL(maxpool3x3s2_valid_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, N, H, C);
                        return hipGetLastError();
                    }});
    prog.back().out = out; prog.back().out_elems = total * 8; prog.back().out_bf16 = 1;
}

int build_lpips(hd_ctx* c, int B, const float* images, int res, const float* ref, int R, int unit_range, const float* images_range,
                const float* ref_range, double* out, double* layers_out) {
    auto& prog = c->ws->lpips_prog.ops; prog.clear();
    auto& v = c->ws->lws; auto& w = c->lw;
    const int N = 2 * B;
    int s[3];
    lp_sides(R, s);
    {
        uint4* in8 = v.in8; const size_t npix = (size_t)N * R * R; const LpScale sc = w.sc;
        prog.push_back({"input", [=](hipStream_t st) -> hipError_t {
                            hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, images, res, ref, R, B, unit_range,
                                               images_range, ref_range, sc, in8);
                            return hipGetLastError();
                        }});
        prog.back().out = in8; prog.back().out_elems = npix * 8; prog.back().out_bf16 = 1;
    }
    lp_conv(c, prog, kLpOpName[0], w.conv[0], kLpConv[0], reinterpret_cast<const unsigned short*>(v.in8), N, R, v.f[0]);
    lp_pool(prog, "slice2.pool", v.f[0], v.pool[0], N, s[0], 64);
    lp_conv(c, prog, kLpOpName[1], w.conv[1], kLpConv[1], v.pool[0], N, s[1], v.f[1]);
    lp_pool(prog, "slice3.pool", v.f[1], v.pool[1], N, s[1], 192);
    lp_conv(c, prog, kLpOpName[2], w.conv[2], kLpConv[2], v.pool[1], N, s[2], v.f[2]);
    lp_conv(c, prog, kLpOpName[3], w.conv[3], kLpConv[3], v.f[2], N, s[2], v.f[3]);
    lp_conv(c, prog, kLpOpName[4], w.conv[4], kLpConv[4], v.f[3], N, s[2], v.f[4]);
    LpDistP d{};
    d.B = B; d.partial = v.part;
    for (int k = 0; k < LP_LAYERS; ++k) {
        const int side = s[k < 2 ? k : 2];
        d.feat[k] = v.f[k]; d.w[k] = w.lin[k]; d.C[k] = kLpConv[k].cout; d.P[k] = side * side;
        d.wg0[k + 1] = d.wg0[k] + (d.P[k] + LP_POS_PER_WG - 1) / LP_POS_PER_WG;
    }
    // the two fp64 outputs are read back (hd_debug_read_op) as their 32-bit words, two per value
    prog.push_back({"distance", [=](hipStream_t st) -> hipError_t {
                        hipLaunchKernelGGL(lpips_distance_kernel, dim3(d.wg0[LP_LAYERS], B), dim3(LP_THREADS), 0, st, d);
                        return hipGetLastError();
                    }});
    prog.back().out = v.part; prog.back().out_elems = (size_t)B * d.wg0[LP_LAYERS] * 2;
    prog.push_back({"combine", [=](hipStream_t st) -> hipError_t {
                        hipLaunchKernelGGL(lpips_combine_kernel, dim3(B), dim3(64), 0, st, d, out, layers_out);
                        return hipGetLastError();
                    }});
    prog.back().out = out; prog.back().out_elems = (size_t)B * 2;
    return HD_OK;
}

}  // namespace

int finalize_lpips(hd_ctx* c) {
    auto man = build_lpips_manifest();
    const bool own_scale = find_raw(c, "scaling_layer.shift") || find_raw(c, "scaling_layer.scale");     // optional, but both or neither
    if (own_scale) { man.push_back({"scaling_layer.shift", {1, 3, 1, 1}}); man.push_back({"scaling_layer.scale", {1, 3, 1, 1}}); }
    if (const int bad = check_manifest(c, man)) return bad;
    auto& w = c->lw;
    PackOpts pad8; pad8.cin_pad = 8;
    for (int k = 0; k < LP_LAYERS; ++k) {
        if (const int rc = pack_weight(c, kLpConv[k].name, &w.conv[k], k == 0 ? pad8 : PackOpts())) return rc;
        w.lin[k] = find_raw(c, "lin" + std::to_string(k) + ".model.1.weight")->dev;
    }
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    for (int i = 0; i < 3; ++i) {
        w.sc.shift[i] = own_scale ? find_raw(c, "scaling_layer.shift")->host[i] : shift[i];
        w.sc.scale[i] = own_scale ? find_raw(c, "scaling_layer.scale")->host[i] : scale[i];
        if (!(std::fabs(w.sc.scale[i]) > 0.f) || !std::isfinite(w.sc.scale[i]) || !std::isfinite(w.sc.shift[i]))
            HD_FAIL(c, HD_ERR_WEIGHTS, "scaling_layer: scale must be finite and non-zero, shift finite (channel %d)", i);
    }
    HIPCHECK(c, hipDeviceSynchronize());
    c->finalized = true;
    return HD_OK;
}

extern "C" {

int hd_lpips_create(hd_ctx** out, int device) {
    int rc = hd_create(out, 16, device);
    if (rc == HD_OK) { (*out)->lpips = true; (*out)->conditional = false; }
    return rc;
}

int hd_lpips(hd_ctx* c, int batch, const float* images, int res, const float* ref, int ref_res, int unit_range, const float* images_range,
             const float* ref_range, double* out, double* layers_out, void* stream) {
    if (!c) return HD_ERR_INVALID;
    if (!c->lpips) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: ctx is not an LPIPS context (hd_lpips_create)");
    if (!c->finalized) HD_FAIL(c, HD_ERR_NOT_READY, "hd_lpips: ctx has no finalized weights (hd_load_weights / hd_finalize_weights)");
    if (batch < 1 || batch > 1024) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: batch must be in [1, 1024], got %d", batch);
    if (!res_ok(res)) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: res must be a multiple of 64 in [64, 512], got %d", res);
    if (!res_ok(ref_res)) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: ref_res must be a multiple of 64 in [64, 512], got %d", ref_res);
    if (unit_range != 0 && unit_range != 1) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: unit_range must be 0 or 1, got %d", unit_range);
    if (!images) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: images is NULL");
    if (!ref) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: ref is NULL");
    if (!out) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: out is NULL");
    const uintptr_t pi = (uintptr_t)images, pr = (uintptr_t)ref, pir = (uintptr_t)images_range, prr = (uintptr_t)ref_range;
    const uintptr_t po = (uintptr_t)out, pl = (uintptr_t)layers_out;
    if ((pi | pr | pir | prr) % sizeof(float)) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: images, ref, images_range and ref_range must be aligned to 4 bytes");
    if ((po | pl) % sizeof(double)) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: out and layers_out must be aligned to 8 bytes");
    const size_t nimg = (size_t)batch * 3 * res * res * sizeof(float), nref = (size_t)batch * 3 * ref_res * ref_res * sizeof(float);
    const size_t nrange = (size_t)batch * 2 * sizeof(float), nout = (size_t)batch * sizeof(double), nlay = nout * LP_LAYERS;
    const ByteRange outs[2] = {{"out", out, nout}, {"layers_out", layers_out, nlay}},
                    ins[4] = {{"images", images, nimg}, {"ref", ref, nref}, {"images_range", images_range, nrange}, {"ref_range", ref_range, nrange}};
    const ByteRange *a, *b;
    if (first_overlap(outs, 2, ins, 4, &a, &b)) HD_FAIL(c, HD_ERR_INVALID, "hd_lpips: %s overlaps %s", a->name, b->name);
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = alloc_lpips(c, batch, ref_res);
    if (rc) return rc;
    CachedProgram& cp = c->ws->lpips_prog;
    const ProgramKey key = {{images, ref, images_range, ref_range, out, layers_out}, (uint64_t)(res * 2 + unit_range)};
    if (!cp.matches(key)) {
        rc = build_lpips(c, batch, images, res, ref, ref_res, unit_range, images_range, ref_range, out, layers_out);
        if (rc) return rc;
        cp.store(key);
    }
    return run_ops(c, cp.ops, reinterpret_cast<hipStream_t>(stream), c->op_limit);
}

}  // extern "C"
