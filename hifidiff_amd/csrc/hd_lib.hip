// hd_lib.hip -- libhifidiff_hip.so: the refiner's context (weights, per-batch workspaces), the denoiser / conditioning launch
// programs, the hipGraph-replayed sampler and the C-ABI of include/hifidiff_hip.h.  Shared internals: hd_internal.hpp;
// CoarseRestoration and the VAE boundary: hd_aux.hip; the persistent stage kernels: hd_stages.hip.
#include "hd_internal.hpp"

static std::string g_create_error;
// what hd_last_error(NULL) returns, for the entry points of hd_aux.hip that take no context (hd_color_fix)
void set_contextless_error(const std::string& msg) { g_create_error = msg; }

namespace {

// --------------------------------------------------------------------------------------- workspace
int alloc_chain(hd_ctx* c, Chain& ch) {
    const int L = c->L, B = ch.B;
    const bool names = (ch.index == 0);                  // introspection reads chain 0
    auto& dbg = c->ws->dbg;
    int rc = 0;
    for (int l = 0; l < 5; ++l) {
        Level& v = ch.lv[l];
        v.C = WIDTH << l; v.H = L >> l; v.M = B * v.H * v.H;
        const size_t mc = (size_t)v.M * v.C;
        rc |= alloc_level(c, v, B, mc, names, l);
        const int pi = 4 - l;                            // prior index: coarsest first
        rc |= ws_alloc(c, &ch.prior[pi], mc); rc |= ws_alloc(c, &ch.gate_c[pi], (size_t)B * v.C);
        rc |= ws_alloc(c, &ch.gate_s[pi], (size_t)v.M);
        if (rc) return rc;
        if (names) {
            const std::string ps = std::to_string(pi);
            dbg["Xg" + std::to_string(l)] = {v.Xg, {mc, 1}};
            dbg["prior" + ps] = {ch.prior[pi], {mc, 0}}; dbg["wc" + ps] = {ch.gate_c[pi], {(size_t)B * v.C, 0}};
            dbg["ws" + ps] = {ch.gate_s[pi], {(size_t)v.M, 0}};
        }
    }
    rc |= ws_alloc(c, &ch.idc_term, (size_t)B * 2048 * c->S * c->S); rc |= ws_alloc(c, &ch.id_emb, (size_t)B * 2048);
    rc |= ws_alloc(c, &ch.pool_tmp, (size_t)B * 2048); rc |= ws_alloc(c, &ch.mlp_tmp, (size_t)B * 2048);
    rc |= ws_alloc(c, &ch.sp_tmp, (size_t)ch.lv[0].M * 1024);       // >= max over levels of M_l * C_l / 2
    if (rc) return rc;
    if (names) { dbg["idc"] = {ch.idc_term, {(size_t)B * 2048 * c->S * c->S, 0}}; dbg["id_emb"] = {ch.id_emb, {(size_t)B * 2048, 0}}; }
    // ResNet activations (channels-last bf16); largest is conv1 output B x 64x64 x 64 == layer1 B x 32x32 x 256
    const size_t rmax = (size_t)B * 64 * 64 * 64;
    for (int i = 0; i < 4; ++i) rc |= ws_alloc(c, &ch.res_buf[i], rmax);
    rc |= ws_alloc(c, &ch.face8, (size_t)B * 128 * 128);
    rc |= ws_alloc(c, &ch.step_state, 1);
    rc |= ws_alloc(c, &ch.film_cur, (size_t)c->film_total);
    if (rc) return rc;
    HIPCHECK(c, hipMemset(ch.step_state, 0, sizeof(StepState)));
    HIPCHECK(c, hipStreamCreateWithFlags(&ch.stream, hipStreamNonBlocking));
    HIPCHECK(c, hipEventCreateWithFlags(&ch.done, hipEventDisableTiming));
    return HD_OK;
}

int build_denoiser_program(hd_ctx* c);
int get_xstage(hd_ctx* c, int first_block, int nblocks, hd_ctx::XStage** out);
// diffusion steps per captured graph (kGraphSteps; HD_GRAPH_STEPS under HD_EXPERIMENTS=1 measures other lengths)
static int graph_steps() {
    static const int v = [] { const char* e = hd_env("HD_GRAPH_STEPS"); const int n = e ? atoi(e) : kGraphSteps; return n < 1 ? 1 : (n > 250 ? 250 : n); }();
    return v;
}
int setup_xcd(hd_ctx* c);

// Cut the batch into chains (HD_CHAINS, default 1).  Two streams of these kernels do overlap (1.6x in
// tools/gemm_bench), but halving M does not make a kernel cheaper, so splitting the batch is not a win.
int alloc_workspace_new(hd_ctx* c, Workspace& w, int B) {
    int n = 1;                                            // measured: per-kernel cost barely depends on M, so more chains only add launches
    if (const char* e = hd_env("HD_CHAINS")) n = atoi(e);         // experiment switch (needs HD_EXPERIMENTS=1): measured slower at 2 and 4
    if (n < 1) n = 1;
    if (n > 8) n = 8;
    while (n > 1 && B % n != 0) --n;
    const size_t per_face = (size_t)4 * c->L * c->L;
    int rc = 0;
    rc |= ws_alloc(c, &w.lat, (size_t)B * per_face); rc |= ws_alloc(c, &w.eps, (size_t)B * per_face);
    rc |= ws_alloc(c, &w.x0_hist, (size_t)B * per_face);
    if (rc) return rc;
    w.dbg["lat"] = {w.lat, {(size_t)B * per_face, 0}}; w.dbg["eps"] = {w.eps, {(size_t)B * per_face, 0}};
    w.dbg["x0_hist"] = {w.x0_hist, {(size_t)B * per_face, 0}};
    w.chains.resize(n);
    for (int i = 0; i < n; ++i) {
        Chain& ch = w.chains[i];
        ch.index = i; ch.B = B / n; ch.face0 = i * (B / n);
        ch.lat = w.lat + (size_t)ch.face0 * per_face; ch.eps = w.eps + (size_t)ch.face0 * per_face;
        ch.x0_hist = w.x0_hist + (size_t)ch.face0 * per_face;
        rc = alloc_chain(c, ch);
        if (rc) return rc;
    }
    w.B = B;
    for (auto& ch : w.chains) {
        ChainCursor on(c, &ch);
        rc = build_denoiser_program(c);
        if (rc) return rc;
    }
    return HD_OK;
}
// another batch size: the buffers, programs and graphs of the one in use are kept for later
int alloc_workspace(hd_ctx* c, int B) {
    return switch_workspace(c, B, [&](Workspace& w) { return alloc_workspace_new(c, w, B); });
}

// ----------------------------------------------------------------------------- program construction
int build_denoiser_program(hd_ctx* c) {
    std::vector<Op>& prog = c->ch->program;
    prog.clear();
    const int B = c->ch->B, L = c->L;
    Chain* chp = c->ch;
    const RawTensor *iw = find_raw(c, "denoiser.intro.weight"), *ib = find_raw(c, "denoiser.intro.bias");
    const RawTensor *ew = find_raw(c, "denoiser.ending.weight"), *eb = find_raw(c, "denoiser.ending.bias");
    // The intro conv: a launch of its own, or -- latent 16, batch <= 64, face-cluster stages available -- the ENTRY of the level-0 encoder stage
    // (hd_face.hpp: every workgroup computes x of its own and halo image rows from the latents; one launch less per step).  The launch stays as
    // the first step of that stage's per-GEMM form.
    std::function<hipError_t(hipStream_t)> intro_run;
    {
        const float *lat = c->ch->lat, *w = c->intro_wT, *b = ib->dev; float* out = c->ch->lv[0].X; float2* sx = c->ch->lv[0].sx;
        unsigned short* xb = c->ch->lv[0].Xb;
        const int M = c->ch->lv[0].M;
        intro_run = [=](hipStream_t s) -> hipError_t {
            if (M >= kLongRunRows) hipLaunchKernelGGL(intro_conv_kernel<16>, dim3((M / 16 + 3) / 4), dim3(256), 0, s, lat, w, b, out, xb, sx, B, L, chp->step_state, mode_is_loop(c->mode));
            else hipLaunchKernelGGL(intro_conv_kernel<kIntroPx>, dim3((M / kIntroPx + 3) / 4), dim3(256), 0, s, lat, w, b, out, xb, sx, B, L, chp->step_state, mode_is_loop(c->mode));
            return hipGetLastError();
        };
    }
    const bool fold_intro = c->xcd_ok && c->face_ok && c->intro_fold && B <= 64 && L == 16 && c->ch->lv[0].C == 128 && c->ch->lv[0].H == 16;
    if (!fold_intro) {
        prog.push_back({"intro", intro_run});
        prog.back().out = c->ch->lv[0].X; prog.back().out_elems = (size_t)c->ch->lv[0].M * 128;
    }
    const int enc[4] = {2, 2, 4, 8};
    int bi = 0;
    int np = 1, cnt = WIDTH;                            // intro emits one (mean, M2) partial per row
    // A run of blocks of one level: as per-GEMM launches, and -- levels 2 and 3 at latent 16, batch <= 64 -- as ONE
    // XCD-local persistent launch (hd_xcd.hpp) when its conditions hold at run time (a single chain: every workgroup
    // must be resident; one FiLM row for all faces).  Both forms compute the same bits.
    int stage_rc = HD_OK;
    auto add_stage = [&](int nblk, const Level& lv, const GateOut* gate) {
        const int first = bi;
        const bool shape_ok = c->xcd_ok && B <= XS_GROUPS * XS_FACES && np == lv.C / 32 && cnt == 32 &&
                              ((lv.C == 1024 && lv.H == 2) || (lv.C == 512 && lv.H == 4)) && nblk <= XS_MAXBLK;
        auto sub = std::make_shared<std::vector<Op>>();
        for (int j = 0; j < nblk; ++j)
            add_naf_block(c, shape_ok ? *sub : prog, c->den_blocks[bi++], lv, nullptr, &np, &cnt, (gate && j == nblk - 1) ? gate : nullptr);
        if (!shape_ok) return;
        hd_ctx::XStage* xs = nullptr;
        stage_rc = get_xstage(c, first, nblk, &xs);
        if (stage_rc) return;
        XStageP sp{};
        sp.B = B; sp.nblocks = nblk; sp.blocks = xs->blocks_dev;
        sp.X = lv.X; sp.Xb = lv.Xb; sp.sx = lv.sx; sp.G = lv.G; sp.Yb = lv.Yb; sp.sy = lv.sy;
        sp.pooled16 = lv.pooled16; sp.pooled = lv.pooled; sp.S = lv.S; sp.ln_eps = 1e-6f;
        if (gate) { sp.outg16 = lv.Xg; sp.gate_c = gate->gate_c; sp.gate_s = gate->gate_s; sp.add_src = gate->add; }
        sp.flags = xs->sync; sp.hello = xs->sync + 256; sp.gstate = xs->sync + 512; sp.tmo = c->xcd_tmo_dev; sp.abort_dev = c->abort_dev;
        const bool l3 = lv.C == 1024;
        X2StageP sp2{};
        if (xs->blocks2_dev) {
            sp2.B = B; sp2.nblocks = nblk; sp2.blocks = xs->blocks2_dev;
            sp2.X = lv.X; sp2.Xb = lv.Xb; sp2.sx = lv.sx; sp2.hX = xs->hX; sp2.hG = xs->hG; sp2.hY = xs->hY; sp2.hsx = xs->hsx; sp2.hsy = xs->hsy;
            sp2.pooled16 = lv.pooled16; sp2.dG = lv.G; sp2.dYb = lv.Yb; sp2.dpooled = lv.pooled; sp2.dS = lv.S; sp2.ln_eps = 1e-6f;
            if (gate) { sp2.outg16 = lv.Xg; sp2.gate_c = gate->gate_c; sp2.gate_s = gate->gate_s; sp2.add_src = gate->add; }
            sp2.flags = xs->sync2; sp2.hello = xs->sync2 + 1024; sp2.gstate = xs->sync2 + 1280; sp2.tmo = c->xcd_tmo_dev; sp2.abort_dev = c->abort_dev;
        }
        const bool have2 = xs->blocks2_dev != nullptr;
        Op op;
        op.name = c->den_blocks[first + nblk - 1].name + ".conv5"; op.out = lv.X; op.out_elems = (size_t)lv.M * lv.C; op.out_bf16 = 0;
        op.run = [c, chp, sp, sp2, have2, sub, l3, first](hipStream_t s) -> hipError_t {
            if (have2 && c->xcd_ok && c->xcd_on && c->xcd2_on && c->ws->chains.size() == 1 && mode_shared_row(c->mode)) {
                X2StageP r = sp2;
                r.film = film_rows(c, chp).base;
                r.phase_limit = (c->stage_limit_first < 0 || c->stage_limit_first == first) ? c->xcd_phase_limit : 0;
                r.force_global = c->xcd_force_global; r.test_abort = c->stage_test_abort;
                const hipError_t e = run_xcd2_stage(l3 ? 1024 : 512, r, s);
                if (e == hipSuccess) { ++c->stage_count; return e; }
                (void)hipGetLastError();                      // refused launch (LDS / CU budget of this device or tenant): nothing ran -> the K-split form, then the per-GEMM launches
                c->xcd2_on = false;
            }
            // (per-face rows of hd_sample_rows*: the K-split form's per-face instantiation; the autonomous-wave form above has none)
            if (c->xcd_ok && c->xcd_on && c->ws->chains.size() == 1 && mode_allows_stages(c->mode)) {
                XStageP r = sp;
                set_film(r, c, chp);
                r.phase_limit = (c->stage_limit_first < 0 || c->stage_limit_first == first) ? c->xcd_phase_limit : 0;
                r.force_global = c->xcd_force_global; r.test_abort = c->stage_test_abort;
                const hipError_t e = mode_is_rows(c->mode) ? run_xcd_rows_stage(l3 ? 1024 : 512, r, s) : run_xcd_stage(l3 ? 1024 : 512, r, s);
                if (e == hipSuccess) { ++c->stage_count; return e; }
                (void)hipGetLastError();                      // as the face stages below: a refused launch is recoverable
                c->xcd_on = false;
            }
            for (auto& o : *sub) { const hipError_t e = o.run(s); if (e != hipSuccess) return e; }
            return hipSuccess;
        };
        prog.push_back(op);
    };
    // Levels 0 / 1 (latent 16, batch <= 64): a run of blocks as ONE launch with the rows of a face split over a cluster of
    // workgroups (hd_face.hpp); the per-block launches (fused conv1 + chain kernel) stay as the other form of the same op.
    auto add_face_stage = [&](int nblk, const Level& lv, const GateOut* gate, bool want_xb, bool with_intro = false, const Op* down_op = nullptr,
                              const Op* up_op = nullptr, const unsigned short* up_A = nullptr) {
        const int first = bi;
        const bool shape_ok = c->xcd_ok && c->face_ok && B <= 64 && ((lv.C == 128 && lv.H == 16) || (lv.C == 256 && lv.H == 8)) && nblk <= XS_MAXBLK && !(gate && gate->add);
        auto sub = std::make_shared<std::vector<Op>>();
        for (int j = 0; j < nblk; ++j)
            add_naf_block(c, shape_ok ? *sub : prog, c->den_blocks[bi++], lv, nullptr, &np, &cnt, (gate && j == nblk - 1) ? gate : nullptr);
        if (!shape_ok) return;
        hd_ctx::XStage* xs = nullptr;
        stage_rc = get_xstage(c, first, nblk, &xs);
        if (stage_rc) return;
        hd_ctx::FStage& fs = c->fstages[first];
        if (!fs.sync) {
            int rc = dev_alloc(c, &fs.sync, (size_t)2 * 64 * 16);
            rc |= dev_alloc(c, &fs.pool_part, (size_t)64 * 8 * 256);
            if (rc || hipMemset(fs.sync, 0, (size_t)2 * 64 * 16 * sizeof(unsigned)) != hipSuccess) { stage_rc = HD_ERR_HIP; return; }
        }
        FStageP fp{};
        fp.B = B; fp.nblocks = nblk; fp.blocks = xs->blocks_dev;
        fp.X = lv.X; fp.Xb = want_xb ? lv.Xb : nullptr; fp.ln_eps = 1e-6f;
        if (gate) { fp.outg16 = lv.Xg; fp.gate_c = gate->gate_c; fp.gate_s = gate->gate_s; }
        fp.pool_part = fs.pool_part; fp.flags = fs.sync; fp.gstate = fs.sync + 64 * 16; fp.tmo = c->xcd_tmo_dev; fp.abort_dev = c->abort_dev;
        const bool c128 = lv.C == 128;
        // the intro conv as this stage's entry (the program then has no intro launch: it is the first step of the per-GEMM form below)
        // (level 1: the same for the down conv of level 0)
        const std::function<hipError_t(hipStream_t)> intro_first = with_intro ? intro_run : down_op ? down_op->run : up_op ? up_op->run : std::function<hipError_t(hipStream_t)>();
        if (up_op) { fp.up_A = up_A; fp.up_W = c->den_up[3].w; }        // level 0's decoder stage: the last up conv (X holds the encoder skip)
        if (with_intro) { fp.intro_lat = chp->lat; fp.intro_wT = c->intro_wT; fp.intro_b = ib->dev; fp.intro_step = &chp->step_state->step; }
        if (down_op) { fp.down_A = c->ch->lv[0].Xb; fp.down_W = c->den_down[0].w; fp.down_b = c->den_down[0].bias; }
        Op op;
        op.name = c->den_blocks[first + nblk - 1].name + ".conv5"; op.out = lv.X; op.out_elems = (size_t)lv.M * lv.C; op.out_bf16 = 0;
        op.run = [c, chp, fp, sub, c128, first, intro_first](hipStream_t s) -> hipError_t {
            // (hd_eps's per-face timesteps and split batches run the per-GEMM form: every workgroup resident is what the stage needs; the
            // per-face rows of hd_sample_rows* have an instantiation of their own)
            if (c->xcd_ok && c->face_on && c->ws->chains.size() == 1 && mode_allows_stages(c->mode)) {
                FStageP r = fp;
                set_film(r, c, chp);
                r.block_limit = (c->stage_limit_first < 0 || c->stage_limit_first == first) ? c->face_block_limit : 0;
                r.test_abort = c->stage_test_abort;
                r.intro_advance = mode_is_loop(c->mode);
                const hipError_t e = mode_is_rows(c->mode) ? run_face_rows_stage(c128 ? 128 : 256, c128 ? 32 : c->face_l1_rows, r, s)
                                                           : run_face_stage(c128 ? 128 : 256, c128 ? 32 : c->face_l1_rows, r, s);
                if (e == hipSuccess) { ++c->stage_count; ++c->face_stage_count; return e; }
                (void)hipGetLastError();                      // (the dynamic-LDS grant was refused: nothing was launched) -> the per-block launches
                c->face_on = false;
            }
            if (intro_first) { const hipError_t e = intro_first(s); if (e != hipSuccess) return e; }
            for (auto& o : *sub) { const hipError_t e = o.run(s); if (e != hipSuccess) return e; }
            return hipSuccess;
        };
        prog.push_back(op);
        np = lv.C / 32; cnt = 32;
    };
    // the down conv of level 0 as the entry of the level-1 stage (same conditions as that stage; HD_NO_DOWN_FOLD=1 keeps the launch)
    // (only the 16-row instantiation of that stage has the entry: HD_FACE_L1_ROWS=32 keeps the launch)
    const bool fold_down0 = fold_intro && c->down_fold && c->face_l1_rows == 16 && c->ch->lv[1].C == 256 && c->ch->lv[1].H == 8 && c->den_down[0].K == 512 && c->den_down[0].N == 256;
    chp->fold_intro = fold_intro; chp->fold_down0 = fold_down0;
    std::vector<Op> down0;
    for (int l = 0; l < 4; ++l) {
        if (l >= 2) add_stage(enc[l], c->ch->lv[l], nullptr);
        else add_face_stage(enc[l], c->ch->lv[l], nullptr, true, l == 0 && fold_intro, (l == 1 && fold_down0) ? &down0[0] : nullptr);
        if (stage_rc) return stage_rc;
        add_down(c, (l == 0 && fold_down0) ? down0 : prog, "downs." + std::to_string(l), c->den_down[l], c->ch->lv[l], c->ch->lv[l + 1]);
        np = c->ch->lv[l + 1].C / 32; cnt = 32;
    }
    // x + idc_conv(id) -> HCA0 (model.py:245-247): the add and the gate are applied by the last mid block's conv5 epilogue.
    // The unconditional Denoiser (model.py:117-128) has neither: the up-convs read the blocks' own bf16 output.
    const bool cond = c->conditional;
    for (int j = 0; j < 8; ++j) {
        GateOut g0; g0.gate_c = c->ch->gate_c[0]; g0.gate_s = c->ch->gate_s[0]; g0.add = c->ch->idc_term;
        add_naf_block(c, prog, c->den_blocks[bi++], c->ch->lv[4], nullptr, &np, &cnt, (cond && j == 7) ? &g0 : nullptr);
    }
    if (cond) add_hca(c, prog, "hcas.0", c->hca[0], c->ch->lv[4].Xg, c->ch->lv[4].Y, c->ch->lv[4].Yb, c->ch->lv[4].M, c->ch->lv[4].H);
    // (with the other folds: the program of the persistent stages; the one-launch-per-GEMM programs keep every launch and its tap)
    const bool fuse_end = cond && fold_intro && c->end_fold && L == 16 && c->ch->lv[0].C == 128 && c->ch->lv[0].H == 16 && !c->hca[4].centre_only;
    chp->fuse_end = fuse_end;
    std::vector<Op> hca4;
    for (int i = 0; i < 4; ++i) {
        const int l = 3 - i;
        const Level &hi = c->ch->lv[l + 1], &lo = c->ch->lv[l];
        // x = PixelShuffle(up(x)) + enc_skip (model.py:249-251); the epilogue also leaves the bf16 copy and the
        // LayerNorm partials of the new rows (one per 32 channels)
        // the last up conv as the entry of the level-0 decoder stage (same conditions as that stage; HD_NO_UP_FOLD=1 keeps the launch)
        const bool fold_up = i == 3 && fold_intro && c->up_fold && lo.C == 128 && lo.H == 16 && c->den_up[3].K == 256 && c->den_up[3].N == 512;
        std::vector<Op> up3;
        if (i == 3) chp->fold_up = fold_up;
        add_up(c, fold_up ? up3 : prog, "ups." + std::to_string(i), c->den_up[i], cond ? hi.Yb : hi.Xb, true, hi.M, hi.H, hi.C, lo.X, lo.X, 2, lo.Xb, lo.sx);
        np = lo.C / 32; cnt = 32;
        GateOut g; g.gate_c = c->ch->gate_c[i + 1]; g.gate_s = c->ch->gate_s[i + 1];
        if (l >= 2) {
            add_stage(2, lo, cond ? &g : nullptr);
            if (stage_rc) return stage_rc;
        } else {
            // unconditional: the up conv / ending read the blocks' own output
            add_face_stage(2, lo, cond ? &g : nullptr, !cond, false, nullptr, fold_up ? &up3[0] : nullptr, cond ? hi.Yb : hi.Xb);
            if (stage_rc) return stage_rc;
        }
        // the last HCA conv and the ending conv as ONE launch (hd_end.hpp; latent 16, conditional refiner; HD_NO_END_FOLD=1 keeps the two launches):
        // the HCA op is then the first step of the ending op's two-launch form
        if (cond) add_hca(c, (i == 3 && fuse_end) ? hca4 : prog, "hcas." + std::to_string(i + 1), c->hca[i + 1], lo.Xg, lo.Y, i < 3 ? lo.Yb : nullptr, lo.M, lo.H);
    }
    {
        const float *X = cond ? c->ch->lv[0].Y : c->ch->lv[0].X, *w = c->ending_wT, *b = eb->dev; float* eps = c->ch->eps;
        const int M = c->ch->lv[0].M;
        Chain* chp = c->ch;
        EndP ep{};
        std::function<hipError_t(hipStream_t)> hca4_run;
        if (fuse_end) {
            ep.B = B; ep.Xg = c->ch->lv[0].Xg; ep.W = c->hca[4].fused.w; ep.bias = c->hca[4].fused.bias; ep.ewT = w; ep.eb = b; ep.eps = eps;
            hca4_run = hca4[0].run;
        }
        // sampling loop: the ending launch also applies the scheduler update to this chain's latents and stages the next step's FiLM
        // row -- per-face rows: every face of this chain stages its own (all zero outside the loop: nothing but the conv)
        auto sched_args = [c, chp, L]() {
            SchedArgs sa{};
            if (!mode_is_loop(c->mode)) return sa;
            const size_t per_face = (size_t)4 * L * L;
            sa.lat = chp->lat; sa.coef = c->coef_dev; sa.st = chp->step_state;
            sa.elem0 = (int)(chp->face0 * per_face); sa.n_total = (int)(c->ws->B * per_face);
            sa.film_table = c->film_table; sa.film_total = c->film_total;
            sa.film_cur = mode_is_rows(c->mode) ? c->film_pf + (size_t)chp->face0 * c->film_total : chp->film_cur;
            return sa;
        };
        // the ending launch; while guidance is switched on (hd_guide_config) the loop's step ends with guided_update_kernel behind it
        auto ending_run = [=](hipStream_t s) -> hipError_t {
                            const bool rows = mode_is_rows(c->mode);
                            if (fuse_end && c->end_fused) {
                                EndP q = ep;
                                q.sa = sched_args();
                                const hipError_t e = launch_hca_ending(q, s, rows);
                                if (e == hipSuccess) return e;
                                (void)hipGetLastError();              // the dynamic-LDS grant was refused: nothing was launched -> the two launches
                                c->end_fused = false;
                            }
                            if (hca4_run) { const hipError_t e = hca4_run(s); if (e != hipSuccess) return e; }
                            const bool long_runs = M >= kLongRunRows;
                            unsigned nb = (unsigned)((M / (long_runs ? 16 : kEndingPx) + 3) / 4);
                            const SchedArgs sa = sched_args();
                            if (rows) {                               // the workgroups behind the conv's stage the next row(s)
                                nb += (unsigned)(B * film_stage_pieces(c->film_total));
                                if (long_runs) hipLaunchKernelGGL((ending_conv_kernel<16, true>), dim3(nb), dim3(256), 0, s, X, w, b, eps, B, L, sa);
                                else hipLaunchKernelGGL((ending_conv_kernel<kEndingPx, true>), dim3(nb), dim3(256), 0, s, X, w, b, eps, B, L, sa);
                                return hipGetLastError();
                            }
                            if (mode_is_loop(c->mode)) nb += (unsigned)((c->film_total / 4 + 255) / 256);
                            if (long_runs) hipLaunchKernelGGL(ending_conv_kernel<16>, dim3(nb), dim3(256), 0, s, X, w, b, eps, B, L, sa);
                            else hipLaunchKernelGGL(ending_conv_kernel<kEndingPx>, dim3(nb), dim3(256), 0, s, X, w, b, eps, B, L, sa);
                            return hipGetLastError();
                        };
        prog.push_back({"ending", [=](hipStream_t s) -> hipError_t {
                            const hipError_t e = ending_run(s);
                            if (e != hipSuccess || !c->guide.on || !mode_is_loop(c->mode)) return e;
                            const SchedArgs sa = sched_args();
                            GuideArgs g{};
                            g.lat = sa.lat; g.eps = eps; g.coef = sa.coef; g.st = sa.st; g.elem0 = sa.elem0; g.n_total = sa.n_total; g.L = L;
                            if (mode_is_rows(c->mode)) hipLaunchKernelGGL(guided_update_kernel<true>, dim3(B * 4), dim3(256), guide_lds_bytes(L), s, g);
                            else hipLaunchKernelGGL(guided_update_kernel<false>, dim3(B * 4), dim3(256), guide_lds_bytes(L), s, g);
                            return hipGetLastError();
                        }});
        prog.back().out = eps; prog.back().out_elems = (size_t)B * 4 * L * L;
    }
    link_prefetch(prog, true);
    return HD_OK;
}

// HCA gates from prior maps (hca.py:33-48): w_c -> gate_c[i], w_s -> gate_s[i]
void add_gates(hd_ctx* c, std::vector<Op>& prog, int i) {
    const Level& lv = c->ch->lv[4 - i];
    const HcaW& hw = c->hca[i];
    const int C = hw.C, HW = lv.H * lv.H, B = c->ch->B, M = lv.M;
    const float* prior = c->ch->prior[i];
    float *pool = c->ch->pool_tmp, *mlp = c->ch->mlp_tmp, *sp = c->ch->sp_tmp, *gc = c->ch->gate_c[i], *gs = c->ch->gate_s[i];
    const std::string n = "hcas." + std::to_string(i);
    prog.push_back({n + ".pool", [=](hipStream_t s) -> hipError_t {
                        hipLaunchKernelGGL(pool_avgmax_kernel, dim3((C + 255) / 256, B), dim3(256), 0, s, prior, pool, HW, C);
                        return hipGetLastError();
                    }});
    prog.back().out = pool; prog.back().out_elems = (size_t)B * C;
    { GemmP p = base_gemm(hw.mlp0, B); p.A = pool; p.lda = C; p.out = mlp; p.ldo = C; p.act = 1; add_gemm(c, prog, n + ".channel_mlp.0", p, LK_F32, EK_BIASF32); }
    { GemmP p = base_gemm(hw.mlp2, B); p.A = mlp; p.lda = C; p.out = gc; p.ldo = C; p.act = 2; add_gemm(c, prog, n + ".channel_mlp.2", p, LK_F32, EK_BIASF32); }
    { GemmP p = base_gemm(hw.sp0, M); p.A = prior; p.lda = C; p.out = sp; p.ldo = C / 2; p.act = 1; add_gemm(c, prog, n + ".spatial_mlp.0", p, LK_F32, EK_BIASF32); }
    {
        const float* w3 = hw.sp3_w; const float b3 = hw.sp3_b;
        prog.push_back({n + ".spatial_mlp.3", [=](hipStream_t s) -> hipError_t {
                            hipLaunchKernelGGL(rowdot_sigmoid_kernel, dim3((M + 3) / 4), dim3(256), 0, s, sp, w3, b3, gs, M, C / 2);
                            return hipGetLastError();
                        }});
        prog.back().out = gs; prog.back().out_elems = (size_t)M;
    }
}

void add_idc_term(hd_ctx* c, std::vector<Op>& prog) {
    GemmP p = base_gemm(c->idc_conv, c->ch->B);
    p.A = c->ch->id_emb; p.lda = 2048; p.out = c->ch->idc_term; p.ldo = c->idc_conv.N;
    add_gemm(c, prog, "idc_conv", p, LK_F32, EK_BIASF32);
}

void add_fpg(hd_ctx* c, std::vector<Op>& prog, const float* cr_latent_dev) {
    const int B = c->ch->B, L = c->L;
    const RawTensor *iw = find_raw(c, "fpg.intro.weight"), *ib = find_raw(c, "fpg.intro.bias");
    {
        const float *w = c->fpg_intro_wT, *b = ib->dev; float* out = c->ch->lv[0].X; const int M = c->ch->lv[0].M; float2* sx = c->ch->lv[0].sx;
        unsigned short* xb = c->ch->lv[0].Xb;
        Chain* chp = c->ch;
        prog.push_back({"fpg.intro", [=](hipStream_t s) -> hipError_t {
                            if (M >= kLongRunRows) hipLaunchKernelGGL(intro_conv_kernel<16>, dim3((M / 16 + 3) / 4), dim3(256), 0, s, cr_latent_dev, w, b, out, xb, sx, B, L, chp->step_state, 0);
                            else hipLaunchKernelGGL(intro_conv_kernel<kIntroPx>, dim3((M / kIntroPx + 3) / 4), dim3(256), 0, s, cr_latent_dev, w, b, out, xb, sx, B, L, chp->step_state, 0);
                            return hipGetLastError();
                        }});
        prog.back().out = out; prog.back().out_elems = (size_t)M * 128;
    }
    const int enc[4] = {2, 2, 4, 8};
    int bi = 0;
    int np = 1, cnt = WIDTH;
    for (int l = 0; l < 4; ++l) {
        for (int j = 0; j < enc[l]; ++j) add_naf_block(c, prog, c->fpg_blocks[bi++], c->ch->lv[l], c->fpg_ln_pack, &np, &cnt);
        add_down(c, prog, "fpg.downs." + std::to_string(l), c->fpg_down[l], c->ch->lv[l], c->ch->lv[l + 1]);
        np = c->ch->lv[l + 1].C / 32; cnt = 32;
    }
    // convs[0]: 1x1, PixelShuffle(1) == identity -> prior0; then 4x (1x1, PixelShuffle(2), + enc skip)
    add_up(c, prog, "fpg.convs.0", c->fpg_convs[0], c->ch->lv[4].X, false, c->ch->lv[4].M, c->ch->lv[4].H, c->ch->lv[4].C, c->ch->prior[0], nullptr, 1);
    for (int i = 1; i < 5; ++i) {
        const Level &hi = c->ch->lv[5 - i], &lo = c->ch->lv[4 - i];
        // out = shuffled + skip: write into prior[i] with the encoder output as the additive source
        GemmP p = base_gemm(c->fpg_convs[i], hi.M);
        p.A = c->ch->prior[i - 1]; p.lda = hi.C; p.Hin = hi.H; p.Win = hi.H; p.shuffle_r = 2;
        p.out = c->ch->prior[i]; p.ldo = lo.C; p.resid = lo.X; p.bias = nullptr;
        add_gemm(c, prog, "fpg.convs." + std::to_string(i), p, LK_F32, EK_PIXSHUF);
    }
}

void add_resconv(hd_ctx* c, std::vector<Op>& prog, const std::string& name, const ResConv& rc, const unsigned short* in, int Hin,
                 unsigned short* out, const unsigned short* resid, bool relu) {
    const int Hout = (Hin + 2 * rc.pad - rc.k) / rc.stride + 1;
    GemmP p = base_gemm(rc.w, c->ch->B * Hout * Hout);
    p.A = in; p.out = out; p.ldo = rc.cout; p.resid = resid; p.ldr = rc.cout; p.act = relu ? 1 : 0;
    if (rc.k == 1 && rc.stride == 1) {
        p.lda = rc.cin;
        add_gemm(c, prog, name, p, LK_BF16, EK_BIASBF16);
    } else {
        const int cin = rc.w.K / (rc.k * rc.k);          // padded Cin
        p.lda = cin; p.Hin = Hin; p.Win = Hin; p.Cin = cin; p.KH = rc.k; p.KW = rc.k; p.stride = rc.stride; p.pad = rc.pad;
        p.Hout = Hout; p.Wout = Hout; p.ntaps = rc.k * rc.k;
        add_gemm(c, prog, name, p, LK_CONV_BF16, EK_BIASBF16);
    }
}

// ResNet-50 trunk (idc/model.py:122-135) on cr_face -> id_emb [B][2048]
void add_resnet(hd_ctx* c, std::vector<Op>& prog, const float* cr_face_dev) {
    const int B = c->ch->B;
    {
        uint4* f8 = c->ch->face8; const size_t npix = (size_t)B * 128 * 128;
        prog.push_back({"idc.input", [=](hipStream_t s) -> hipError_t {
                            hipLaunchKernelGGL(nchw3_to_nhwc8_bf16_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, cr_face_dev, f8, 128 * 128, npix);
                            return hipGetLastError();
                        }});
        prog.back().out = f8; prog.back().out_elems = npix * 8; prog.back().out_bf16 = 1;
    }
    unsigned short *b0 = c->ch->res_buf[0], *b1 = c->ch->res_buf[1], *b2 = c->ch->res_buf[2], *b3 = c->ch->res_buf[3];
    add_resconv(c, prog, "idc.conv1", c->res_conv1, reinterpret_cast<const unsigned short*>(c->ch->face8), 128, b0, nullptr, true);
    {
        const size_t total = (size_t)B * 32 * 32 * 64;
        prog.push_back({"idc.max_pool", [=](hipStream_t s) -> hipError_t {
                            hipLaunchKernelGGL(maxpool3x3s2_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, b0, b1, B, 64, 64, 64);
                            return hipGetLastError();
                        }});
        prog.back().out = b1; prog.back().out_elems = total; prog.back().out_bf16 = 1;
    }
    unsigned short *x = b1, *y1 = b0, *y2 = b2, *idn = b3;
    int H = 32, bi = 0;
    const int res_layers[4] = {3, 4, 6, 3};
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < res_layers[li]; ++b) {
            const ResBlock& rb = c->res_blocks[bi++];
            const std::string q = "idc.layer" + std::to_string(li + 1) + "." + std::to_string(b);
            const int Hout = H / rb.c2.stride;
            add_resconv(c, prog, q + ".conv1", rb.c1, x, H, y1, nullptr, true);
            add_resconv(c, prog, q + ".conv2", rb.c2, y1, H, y2, nullptr, true);
            const unsigned short* identity = x;
            if (rb.has_ds) { add_resconv(c, prog, q + ".i_downsample", rb.ds, x, H, idn, nullptr, false); identity = idn; }
            // conv3 + BN + identity -> ReLU, written to y1 (free again), then rotate
            add_resconv(c, prog, q + ".conv3", rb.c3, y2, Hout, y1, identity, true);
            std::swap(x, y1);
            H = Hout;
        }
    {
        float* emb = c->ch->id_emb; const unsigned short* xin = x; const int HW = H * H;
        prog.push_back({"idc.avgpool", [=](hipStream_t s) -> hipError_t {
                            hipLaunchKernelGGL(avgpool_bf16_kernel, dim3(2048 / 256, B), dim3(256), 0, s, xin, emb, HW, 2048);
                            return hipGetLastError();
                        }});
        prog.back().out = emb; prog.back().out_elems = (size_t)B * 2048;
    }
}

// ------------------------------------------------------------------------------------------ FiLM
int ensure_film_rows(hd_ctx* c, int rows) {
    if (rows <= c->film_rows_cap) return HD_OK;
    dev_free(c, c->t_dev); dev_free(c, c->temb_a); dev_free(c, c->temb_b); dev_free(c, c->temb_c); dev_free(c, c->film_table);
    int rc = 0;
    rc |= dev_alloc(c, &c->t_dev, rows); rc |= dev_alloc(c, &c->temb_a, (size_t)rows * 128);
    rc |= dev_alloc(c, &c->temb_b, (size_t)rows * 1024); rc |= dev_alloc(c, &c->temb_c, (size_t)rows * 512);
    rc |= dev_alloc(c, &c->film_table, (size_t)rows * c->film_total);
    if (rc) return rc;
    c->film_rows_cap = rows;
    c->film_valid = false;
    c->dbg["film"] = {c->film_table, {(size_t)rows * c->film_total, 0}};
    c->dbg["temb"] = {c->temb_c, {(size_t)rows * 512, 0}};
    return HD_OK;
}

// t (device, n values) -> FiLM table rows [n][film_total] (gain/bias with LN affine folded)
int compute_film(hd_ctx* c, const float* t_dev, int n, hipStream_t s) {
    const RawTensor *w1 = find_raw(c, "denoiser.time_mlp.1.weight"), *b1 = find_raw(c, "denoiser.time_mlp.1.bias");
    const RawTensor *w3 = find_raw(c, "denoiser.time_mlp.3.weight"), *b3 = find_raw(c, "denoiser.time_mlp.3.bias");
    hipLaunchKernelGGL(time_embed_kernel, dim3((n * 64 + 255) / 256), dim3(256), 0, s, t_dev, c->freq_dev, c->temb_a, n);
    hipLaunchKernelGGL((linear_f32_kernel<false>), dim3(1024 / 64, (n + 63) / 64), dim3(256), 0, s, c->temb_a, 128, w1->dev, b1->dev, c->temb_b, 1024, n, 1024, 128);
    hipLaunchKernelGGL((linear_f32_kernel<true>), dim3(512 / 64, (n + 63) / 64), dim3(256), 0, s, c->temb_b, 1024, w3->dev, b3->dev, c->temb_c, 512, n, 512, 512);
    hipLaunchKernelGGL((linear_f32_kernel<true>), dim3((c->film_total + 63) / 64, (n + 63) / 64), dim3(256), 0, s, c->temb_c, 512, c->film_W, c->film_b,
                       c->film_table, c->film_total, n, c->film_total, FILM_IN);
    hipLaunchKernelGGL(film_fold_kernel, dim3(2048 / 256, (unsigned)c->den_blocks.size(), n), dim3(256), 0, s, c->film_table, c->ln_pack, c->film_blocks_dev, c->film_total);
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}



// XCD-local persistent stages (hd_xcd.hpp): usable when every one of the 256 workgroups gets a CU of its own (8 XCDs x 32
// CUs) and the level geometry is the latent-16 one (4 / 16 pixels per face at levels 3 / 2).  HD_NO_XCD=1 builds the
// program without them.
int setup_xcd(hd_ctx* c) {
    c->xcd_ok = false; c->face_ok = false;
    c->end_fold = getenv("HD_NO_END_FOLD") == nullptr;
    if (c->S != 1 || getenv("HD_NO_XCD")) return HD_OK;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess || prop.multiProcessorCount != XS_GROUPS * XS_GROUP_WG) return HD_OK;
    HIPCHECK(c, hipHostMalloc(reinterpret_cast<void**>(&c->xcd_tmo_host), 64, hipHostMallocMapped));
    c->xcd_tmo_host[0] = 0;
    HIPCHECK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->xcd_tmo_dev), c->xcd_tmo_host, 0));
    if (int rc = dev_alloc(c, &c->abort_dev, 64)) return rc;
    HIPCHECK(c, hipMemset(c->abort_dev, 0, 64 * sizeof(unsigned)));
    c->xcd_ok = true;
    c->xcd2_mask = getenv("HD_XCD2") ? (atoi(getenv("HD_XCD2")) & 3) : 1;
    c->face_ok = getenv("HD_NO_FACE") == nullptr;
    c->intro_fold = getenv("HD_NO_INTRO_FOLD") == nullptr;
    c->down_fold = getenv("HD_NO_DOWN_FOLD") == nullptr;
    c->up_fold = getenv("HD_NO_UP_FOLD") == nullptr;
    if (const char* e = getenv("HD_FACE_L1_ROWS")) c->face_l1_rows = atoi(e) == 32 ? 32 : 16;        // per context, like xcd_ok: not a process-wide static (fixtures toggle the variable around make_model)
    return HD_OK;
}
// the device-side description of a stage (weights only: shared by every workspace), created on first use
int get_xstage(hd_ctx* c, int first_block, int nblocks, hd_ctx::XStage** out) {
    auto it = c->xstages.find(first_block);
    if (it != c->xstages.end() && it->second.nblocks == nblocks) { *out = &it->second; return HD_OK; }
    hd_ctx::XStage st;
    st.nblocks = nblocks;
    std::vector<XBlockW> host((size_t)nblocks);
    for (int j = 0; j < nblocks; ++j) {
        const BlockW& bw = c->den_blocks[first_block + j];
        XBlockW& x = host[j];
        x.w1 = bw.conv1.w; x.wsca = bw.sca.w; x.w3 = bw.conv3.w; x.w4 = bw.conv4.w; x.w5 = bw.conv5.w;
        x.b1 = bw.conv1.bias; x.bsca = bw.sca.bias; x.b3 = bw.conv3.bias; x.b4 = bw.conv4.bias; x.b5 = bw.conv5.bias;
        x.beta = bw.beta; x.gamma = bw.gamma; x.dw_w = bw.dw_wT; x.dw_b = bw.dw_b; x.film_off = bw.film_off; x.pad_ = 0;
    }
    int rc = dev_alloc(c, &st.blocks_dev, (size_t)nblocks);
    rc |= dev_alloc(c, &st.sync, (size_t)3 * 256);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpy(st.blocks_dev, host.data(), host.size() * sizeof(XBlockW), hipMemcpyHostToDevice));
    HIPCHECK(c, hipMemset(st.sync, 0, (size_t)3 * 256 * sizeof(unsigned)));
    const int C = c->den_blocks[first_block].C, HW = (C == 1024) ? 4 : 16;
    if (c->xcd2_mask & (C == 1024 ? 2 : 1)) {
        // the five 1x1 convs of every block once more, in the A-operand order of the 16x16x32 MFMA (hd_xcd2.hpp)
        for (int j = 0; j < nblocks; ++j) {
            const BlockW& bw = c->den_blocks[first_block + j];
            const char* conv[5] = {".conv1", ".sca.1", ".conv3", ".conv4", ".conv5"};
            const uint4** dst[5] = {&host[j].w1, &host[j].wsca, &host[j].w3, &host[j].w4, &host[j].w5};
            for (int k = 0; k < 5; ++k) {
                const RawTensor* w = find_raw(c, bw.name + conv[k] + ".weight");
                if (!w || (int)w->shape[1] != C) HD_FAIL(c, HD_ERR_WEIGHTS, "missing %s%s.weight", bw.name.c_str(), conv[k]);
                const int N = (int)w->shape[0];
                uint4* d = nullptr;
                if (int r2 = dev_alloc(c, &d, (size_t)N * C / 8)) return r2;
                hipLaunchKernelGGL(pack_weight16_kernel, dim3(1024), dim3(256), 0, 0, w->dev, d, N, C);
                *dst[k] = d;
            }
        }
        int r2 = dev_alloc(c, &st.blocks2_dev, (size_t)nblocks);
        r2 |= dev_alloc(c, &st.sync2, (size_t)2048);
        const size_t hn = (size_t)64 * HW * C / 8;
        r2 |= dev_alloc(c, &st.hX, hn); r2 |= dev_alloc(c, &st.hG, hn); r2 |= dev_alloc(c, &st.hY, hn);
        r2 |= dev_alloc(c, &st.hsx, (size_t)64 * HW * (C / 16)); r2 |= dev_alloc(c, &st.hsy, (size_t)64 * HW * (C / 16));
        if (r2) return r2;
        HIPCHECK(c, hipGetLastError());
        HIPCHECK(c, hipMemcpy(st.blocks2_dev, host.data(), host.size() * sizeof(XBlockW), hipMemcpyHostToDevice));
        HIPCHECK(c, hipMemset(st.sync2, 0, (size_t)2048 * sizeof(unsigned)));
        HIPCHECK(c, hipMemset(st.hX, 0, hn * 16)); HIPCHECK(c, hipMemset(st.hG, 0, hn * 16)); HIPCHECK(c, hipMemset(st.hY, 0, hn * 16));
        HIPCHECK(c, hipMemset(st.hsx, 0, (size_t)64 * HW * (C / 16) * 8)); HIPCHECK(c, hipMemset(st.hsy, 0, (size_t)64 * HW * (C / 16) * 8));
    }
    c->xstages[first_block] = st;
    *out = &c->xstages[first_block];
    return HD_OK;
}
// A hand-off wait of a persistent stage gave up (a workgroup was not resident, or a fault).  The call in which that
// happened hands back NaN (poison_if_abort_kernel at its end; the remaining stage launches of that call step aside at
// entry), and the failure is reported by the first check that runs after it -- hd_check() behind the caller's
// synchronisation, or the next hd_eps / hd_sample.  Reported once; the context then runs one launch per GEMM.
static int check_xcd(hd_ctx* c) {
    if (c->xcd_tmo_host && c->xcd_tmo_host[0]) {
        const unsigned code = c->xcd_tmo_host[0];
        (void)hipDeviceSynchronize();                      // the failed call's remaining launches still read the words reset below
        c->xcd_tmo_host[0] = 0;
        if (c->abort_dev) (void)hipMemset(c->abort_dev, 0, 64 * sizeof(unsigned));
        c->xcd_on = false;
        invalidate_step_graphs(c);
        for (auto& kv : c->xstages) {
            (void)hipMemset(kv.second.sync, 0, (size_t)3 * 256 * sizeof(unsigned));
            if (kv.second.sync2) (void)hipMemset(kv.second.sync2, 0, (size_t)2048 * sizeof(unsigned));
        }
        for (auto& kv : c->fstages) (void)hipMemset(kv.second.sync, 0, (size_t)2 * 64 * 16 * sizeof(unsigned));
        c->face_on = false;
        HD_FAIL(c, HD_ERR_HIP, "persistent stage: a hand-off wait gave up (code 0x%x%s); the results of that call are invalid (NaN), "
                               "the context now runs one launch per GEMM", code, c->stage_test_abort ? ", injected by stage_test_abort" : "");
    }
    return HD_OK;
}
// End of hd_eps / hd_sample: NaN into the call's result buffer when a stage gave up during the call.
static int poison_on_abort(hd_ctx* c, float* buf, size_t n, hipStream_t s) {
    if (!c->abort_dev || !c->xcd_ok) return HD_OK;
    hipLaunchKernelGGL(poison_if_abort_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->abort_dev, buf, n);
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}

}  // namespace

// ================================================================================================ C-ABI
extern "C" {

const char* hd_last_error(const hd_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int hd_create_unconditional(hd_ctx** out, int latent_res, int device) {
    int rc = hd_create(out, latent_res, device);
    if (rc == HD_OK) (*out)->conditional = false;
    return rc;
}

int hd_create(hd_ctx** out, int latent_res, int device) {
    if (!out) return HD_ERR_INVALID;
    *out = nullptr;
    // 48 (sides 48, 24, 12, 6, 3) is refused: EpPixShufF32::out_row and sched_from_x0's mask index split a row with shifts and masks
    if (latent_res != 16 && latent_res != 32 && latent_res != 64) {
        g_create_error = "latent_res must be 16, 32 or 64 (level sides must be powers of two), got " + std::to_string(latent_res);
        return HD_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_error = "no HIP device available"; return HD_ERR_HIP; }
    if (device < 0 || device >= ndev) { g_create_error = "device index out of range"; return HD_ERR_INVALID; }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return HD_ERR_HIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return HD_ERR_HIP; }
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        g_create_error = std::string("this library is built for gfx950 (MI355X) only; device is ") + prop.gcnArchName;
        return HD_ERR_INVALID;
    }
    hd_ctx* c = new hd_ctx();
    c->L = latent_res; c->device = device; c->S = latent_res / 16;
    int rc = dev_alloc(c, &c->freq_dev, 64);
    if (rc) { g_create_error = c->err; hd_destroy(c); return rc; }
    float freq[64];
    const float e = (float)(-(std::log(10000.0) / 63.0));       // model.py:25: python double, then fp32 tensor math
    for (int k = 0; k < 64; ++k) freq[k] = expf((float)k * e);
    (void)hipMemcpy(c->freq_dev, freq, sizeof(freq), hipMemcpyHostToDevice);
    (void)hipEventCreate(&c->ev0); (void)hipEventCreate(&c->ev1);
    (void)hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming);
    *out = c;
    return HD_OK;
}

void hd_destroy(hd_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    destroy(*c->ws);
    for (auto& kv : c->ws_cache) destroy(*kv.second);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->film_ev) (void)hipEventDestroy(c->film_ev);
    for (auto& sg : c->stage) { if (sg.ev) (void)hipEventDestroy(sg.ev); if (sg.host) (void)hipHostFree(sg.host); }
    if (c->xcd_tmo_host) (void)hipHostFree(c->xcd_tmo_host);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (auto& kv : c->raw) if (kv.second.dev) (void)hipFree(kv.second.dev);
    for (void* p : c->allocs) if (p) (void)hipFree(p);
    delete c;
}

int hd_load_weights(hd_ctx* c, const hd_tensor_desc* t, int n) {
    if (!c || (!t && n > 0)) return HD_ERR_INVALID;
    if (c->finalized) HD_FAIL(c, HD_ERR_INVALID, "weights already finalized");
    HIPCHECK(c, hipSetDevice(c->device));
    for (int i = 0; i < n; ++i) {
        if (!t[i].name || t[i].ndim < 0 || t[i].ndim > 4) HD_FAIL(c, HD_ERR_INVALID, "bad tensor descriptor %d", i);
        const std::string name = t[i].name;
        RawTensor r;
        r.numel = 1;
        for (int d = 0; d < t[i].ndim; ++d) { r.shape.push_back(t[i].shape[d]); r.numel *= (size_t)t[i].shape[d]; }
        const bool counter = name.size() > 19 && name.compare(name.size() - 19, 19, "num_batches_tracked") == 0;
        if (!counter) {
            if (!t[i].data) HD_FAIL(c, HD_ERR_INVALID, "tensor %s has no data", name.c_str());
            HIPCHECK(c, hipMalloc(reinterpret_cast<void**>(&r.dev), r.numel * sizeof(float) + 256));
            HIPCHECK(c, hipMemcpy(r.dev, t[i].data, r.numel * sizeof(float), t[i].is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
            if (r.numel <= HOST_MIRROR_MAX) {
                r.host.resize(r.numel);
                HIPCHECK(c, hipMemcpy(r.host.data(), t[i].data, r.numel * sizeof(float), t[i].is_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
            }
        }
        auto it = c->raw.find(name);
        if (it != c->raw.end() && it->second.dev) (void)hipFree(it->second.dev);
        c->raw[name] = std::move(r);
    }
    return HD_OK;
}

int hd_finalize_weights(hd_ctx* c) {
    if (!c) return HD_ERR_INVALID;
    if (c->finalized) return HD_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    if (c->cr) return finalize_cr(c);
    if (c->vae) return finalize_vae(c);
    if (c->lpips) return finalize_lpips(c);
    if (const int bad = check_manifest(c, build_manifest(c->L, c->conditional))) return bad;
    int rc = 0;
    // ---- NAF blocks (denoiser in execution order, then FPG) ----
    const int enc[4] = {2, 2, 4, 8};
    std::vector<std::pair<std::string, int>> order;
    for (int l = 0; l < 4; ++l) for (int j = 0; j < enc[l]; ++j) order.push_back({"denoiser.encoders." + std::to_string(l) + "." + std::to_string(j), WIDTH << l});
    for (int j = 0; j < 8; ++j) order.push_back({"denoiser.middle_blks." + std::to_string(j), WIDTH << 4});
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) order.push_back({"denoiser.decoders." + std::to_string(i) + "." + std::to_string(j), WIDTH << (3 - i)});
    int off = 0;
    for (auto& e : order) {
        BlockW bw;
        rc = load_naf_block(c, e.first, e.second, bw);
        if (rc) return rc;
        bw.film_off = off;
        off += 4 * e.second;
        c->den_block_index[e.first] = (int)c->den_blocks.size();
        c->den_blocks.push_back(bw);
    }
    c->film_total = off;
    rc = setup_xcd(c);
    if (rc) return rc;
    off = 0;
    for (int l = 0; l < 4 && c->conditional; ++l)
        for (int j = 0; j < enc[l]; ++j) {
            BlockW bw;
            rc = load_naf_block(c, "fpg.encoders." + std::to_string(l) + "." + std::to_string(j), WIDTH << l, bw);
            if (rc) return rc;
            bw.film_off = off;
            off += 4 * (WIDTH << l);
            c->fpg_blocks.push_back(bw);
        }
    const int fpg_film_total = off;
    // ---- FiLM: concatenated Linear(256,4C) weights/biases, LN affine in table layout ----
    rc |= dev_alloc(c, &c->film_W, (size_t)c->film_total * FILM_IN); rc |= dev_alloc(c, &c->film_b, c->film_total);
    rc |= dev_alloc(c, &c->ln_pack, c->film_total); rc |= dev_alloc(c, &c->fpg_ln_pack, fpg_film_total + 4);
    rc |= dev_alloc(c, &c->film_blocks_dev, c->den_blocks.size());
    if (rc) return rc;
    std::vector<FilmBlock> fbs;
    auto copy_ln = [&](const BlockW& bw, float* dst) -> int {
        const char* names[4] = {".norm1.bias", ".norm1.weight", ".norm2.bias", ".norm2.weight"};
        for (int q = 0; q < 4; ++q)
            HIPCHECK(c, hipMemcpy(dst + bw.film_off + q * bw.C, find_raw(c, bw.name + names[q])->dev, bw.C * sizeof(float), hipMemcpyDeviceToDevice));
        return HD_OK;
    };
    for (const BlockW& bw : c->den_blocks) {
        HIPCHECK(c, hipMemcpy(c->film_W + (size_t)bw.film_off * FILM_IN, find_raw(c, bw.name + ".mlp.1.weight")->dev, (size_t)4 * bw.C * FILM_IN * sizeof(float), hipMemcpyDeviceToDevice));
        HIPCHECK(c, hipMemcpy(c->film_b + bw.film_off, find_raw(c, bw.name + ".mlp.1.bias")->dev, (size_t)4 * bw.C * sizeof(float), hipMemcpyDeviceToDevice));
        rc = copy_ln(bw, c->ln_pack);
        if (rc) return rc;
        fbs.push_back({bw.film_off, bw.C});
    }
    for (const BlockW& bw : c->fpg_blocks) { rc = copy_ln(bw, c->fpg_ln_pack); if (rc) return rc; }
    HIPCHECK(c, hipMemcpy(c->film_blocks_dev, fbs.data(), fbs.size() * sizeof(FilmBlock), hipMemcpyHostToDevice));
    // ---- intro / ending weights re-laid for coalesced per-lane loads ----
    {
        const RawTensor *iw = find_raw(c, "denoiser.intro.weight"), *ew = find_raw(c, "denoiser.ending.weight");
        const RawTensor* fw = c->conditional ? find_raw(c, "fpg.intro.weight") : iw;
        if (!iw || !fw || !ew) HD_FAIL(c, HD_ERR_INVALID, "intro/ending weights missing");
        rc |= dev_alloc(c, &c->intro_wT, 36 * 128); rc |= dev_alloc(c, &c->fpg_intro_wT, 36 * 128); rc |= dev_alloc(c, &c->ending_wT, 9 * 4 * 128);
        if (rc) return rc;
        hipLaunchKernelGGL(intro_weight_layout_kernel, dim3(18), dim3(256), 0, 0, iw->dev, c->intro_wT);
        hipLaunchKernelGGL(intro_weight_layout_kernel, dim3(18), dim3(256), 0, 0, fw->dev, c->fpg_intro_wT);
        hipLaunchKernelGGL(ending_weight_layout_kernel, dim3(18), dim3(256), 0, 0, ew->dev, c->ending_wT);
        HIPCHECK(c, hipGetLastError());
    }
    // ---- downs / ups / fpg convs / idc_conv ----
    for (int i = 0; i < 4; ++i) {
        rc |= pack_weight(c, "denoiser.downs." + std::to_string(i), &c->den_down[i]);
        { PackOpts o; o.S2 = 4; rc |= pack_weight(c, "denoiser.ups." + std::to_string(i) + ".0", &c->den_up[i], o); }   // sub-pixel major (EpPixShufF32)
        if (c->conditional) rc |= pack_weight(c, "fpg.downs." + std::to_string(i), &c->fpg_down[i]);
    }
    for (int i = 0; i < 5 && c->conditional; ++i) { PackOpts o; o.S2 = i ? 4 : 1; rc |= pack_weight(c, "fpg.convs." + std::to_string(i) + ".0", &c->fpg_convs[i], o); }
    if (c->conditional) { PackOpts o; o.S2 = c->S * c->S; rc |= pack_weight(c, "denoiser.idc_conv", &c->idc_conv, o); }
    if (rc) return rc;
    // ---- HCAs ----
    for (int i = 0; i < 5 && c->conditional; ++i) {
        HcaW& h = c->hca[i];
        const std::string p = "denoiser.hcas." + std::to_string(i);
        h.C = (WIDTH << 4) >> i;
        h.centre_only = ((c->L >> (4 - i)) == 1);         // 1x1 map: only the centre tap sees data
        rc |= pack_weight(c, p + ".channel_mlp.0", &h.mlp0); rc |= pack_weight(c, p + ".channel_mlp.2", &h.mlp2);
        { PackOpts o; o.bn = p + ".spatial_mlp.1"; rc |= pack_weight(c, p + ".spatial_mlp.0", &h.sp0, o); }
        { PackOpts o; o.bn = p + ".fused_mlp.1"; o.centre_only = h.centre_only; rc |= pack_weight(c, p + ".fused_mlp.0", &h.fused, o); }
        if (rc) return rc;
        std::vector<float> s, o2;
        rc = bn_affine(c, p + ".spatial_mlp.4", s, o2);
        if (rc) return rc;
        const RawTensor *w3 = find_raw(c, p + ".spatial_mlp.3.weight"), *b3 = find_raw(c, p + ".spatial_mlp.3.bias");
        std::vector<float> wf(w3->numel);
        for (size_t k = 0; k < w3->numel; ++k) wf[k] = w3->host[k] * s[0];
        h.sp3_b = b3->host[0] * s[0] + o2[0];
        rc = upload_vec(c, wf, &h.sp3_w);
        if (rc) return rc;
    }
    // ---- ResNet-50 (conv + BN folded) ----
    auto load_res = [&](const std::string& conv, const std::string& bn, int cin, int cout, int k, int stride, int pad, ResConv& r) -> int {
        PackOpts o; o.bn = bn;
        if (cin == 3) o.cin_pad = 8;
        r.cin = cin; r.cout = cout; r.k = k; r.stride = stride; r.pad = pad;
        return pack_weight(c, conv, &r.w, o);
    };
    if (c->conditional) rc = load_res("idc.conv1", "idc.batch_norm1", 3, 64, 7, 2, 3, c->res_conv1);
    if (rc) return rc;
    if (c->conditional) {
        const int res_layers[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512};
        int cin = 64;
        for (int li = 0; li < 4; ++li)
            for (int b = 0; b < res_layers[li]; ++b) {
                const std::string q = "idc.layer" + std::to_string(li + 1) + "." + std::to_string(b);
                const int stride = (b == 0 && li > 0) ? 2 : 1;
                ResBlock rb;
                rc |= load_res(q + ".conv1", q + ".batch_norm1", cin, planes[li], 1, 1, 0, rb.c1);
                rc |= load_res(q + ".conv2", q + ".batch_norm2", planes[li], planes[li], 3, stride, 1, rb.c2);
                rc |= load_res(q + ".conv3", q + ".batch_norm3", planes[li], planes[li] * 4, 1, 1, 0, rb.c3);
                if (b == 0) { rb.has_ds = true; rc |= load_res(q + ".i_downsample.0", q + ".i_downsample.1", cin, planes[li] * 4, 1, stride, 0, rb.ds); }
                if (rc) return rc;
                c->res_blocks.push_back(rb);
                cin = planes[li] * 4;
            }
    }
    HIPCHECK(c, hipDeviceSynchronize());
    // ---- algorithmic per-step figures of the step-variant denoiser (effective taps only) ----
    int64_t params = 0;
    double macs = 0.0;   // per face
    auto add_w = [&](const PackedW& w, double rows_per_face) { params += (int64_t)w.N * w.K; macs += rows_per_face * (double)w.N * w.K; };
    {
        int bi = 0;
        auto blocks_at = [&](int l, int n) {
            const double hw = (double)(c->L >> l) * (c->L >> l);
            for (int j = 0; j < n; ++j) {
                const BlockW& b = c->den_blocks[bi++];
                add_w(b.conv1, hw); add_w(b.conv3, hw); add_w(b.conv4, hw); add_w(b.conv5, hw); add_w(b.sca, 1.0);
                params += 2 * b.C * 9 + 2 * b.C; macs += hw * 2 * b.C * 9;   // depthwise (nominal taps)
            }
        };
        for (int l = 0; l < 4; ++l) blocks_at(l, enc[l]);
        blocks_at(4, 8);
        for (int i = 0; i < 4; ++i) blocks_at(3 - i, 2);
        for (int l = 0; l < 4; ++l) {
            const double hwd = (double)(c->L >> (l + 1)) * (c->L >> (l + 1));
            add_w(c->den_down[l], hwd);
            add_w(c->den_up[l], (double)(c->L >> (4 - l)) * (c->L >> (4 - l)));
        }
        for (int i = 0; i < 5 && c->conditional; ++i) { const double hw = (double)(c->L >> (4 - i)) * (c->L >> (4 - i)); add_w(c->hca[i].fused, hw); }
        params += 2 * 128 * 36; macs += 2.0 * c->L * c->L * 128 * 36;
    }
    c->weight_bytes_per_step = params * 2;
    c->flops_per_face_step = 2.0 * macs;
    c->finalized = true;
    return HD_OK;
}

static int check_ready(hd_ctx* c, bool need_prepared) {
    if (!c) return HD_ERR_INVALID;
    if (!c->finalized) HD_FAIL(c, HD_ERR_NOT_READY, "weights are not loaded/finalized");
    if (need_prepared && !c->prepared) HD_FAIL(c, HD_ERR_NOT_READY, "hd_prepare has not been called for this batch");
    return HD_OK;
}

static int prepare_common(hd_ctx* c, int batch) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (batch <= 0 || batch > 4096) HD_FAIL(c, HD_ERR_INVALID, "batch must be in [1, 4096]");
    HIPCHECK(c, hipSetDevice(c->device));
    return alloc_workspace(c, batch);
}

// ---------------------------------------------------------------------------------- per-face extras: masks, guidance, previews, history
// What each event does to each feature (MaskState, GuideState, PreviewState, HistState in hd_internal.hpp).  Two functions state it:
// extras_clear_all (every hd_prepare*) and extras_clear_slots (a slot refill: hd_prepare_slots, hd_pool_commit); a further per-face
// feature joins each_extra (hd_internal.hpp) and gets a column here.
//   event             c->mask                  c->guide                      c->preview                               c->hist
//   hd_prepare*       every face: no mask      every face: not guided        every face: rows -1, zeroed planes;      valid = false, no face has a history
//                                                                            planes reallocated when the batch or
//                                                                            the snapshot count has changed
//   slot refill       its slots: no mask       its slots: not guided         its slots: rows -1, zeroed planes        its slots: no history; valid = false
//   config off        (no switch)              hd_guide_config(0): every     hd_preview_config(0): planes freed       (no switch)
//                                              face, as hd_prepare*
//   hd_sample*        kept, read               kept, read                    written                                  rewritten (record_history)
//   hd_pool_prepare   nothing                  nothing                       nothing                                  nothing
// A clear launches device work only when a flag was set (the previews have no flags: theirs always runs while they are on).
static int extras_clear_all(hd_ctx* c, hipStream_t s) { return each_extra(c, [&](auto& x) { return x.clear_all(c, s); }); }
// the slot list is on the device already (the first n of ws->slots_dev); the flags are cleared in stream order
static int extras_clear_slots(hd_ctx* c, int n, const int32_t* slots, hipStream_t s) {
    return each_extra(c, [&](auto& x) { return x.clear_slots(c, n, slots, c->ws->slots_dev, s); });
}
static bool extras_active(hd_ctx* c) {
    bool any = false;
    each_extra(c, [&](auto& x) { any |= x.active(c); return HD_OK; });
    return any;
}

// The slots' flags of a set that is valid for the batch go to 0; was one of them set?
static bool unset_slots(FaceSet& fs, int B, int n, const int32_t* slots) {
    bool any = false;
    for (int j = 0; j < n && fs.valid_for(B); ++j) { any |= fs.get(slots[j]); fs.set(slots[j], false); }
    return any;
}
bool MaskState::active(const hd_ctx* c) const { return faces.any(c->ws->B); }
void MaskState::fill(const hd_ctx* c, StepState& st, size_t f0) const {
    const size_t ll = (size_t)c->L * c->L;
    st.mask = dmask + f0 * ll; st.mask_known = dknown + f0 * 4 * ll;
    st.mask_noise = dnoise + f0 * 4 * ll; st.mask_on = on + f0;
}
int MaskState::clear_all(hd_ctx* c, hipStream_t s) {
    if (faces.count() > 0) HIPCHECK(c, hipMemsetAsync(on, 0, (size_t)cap * sizeof(int), s));
    faces.drop();
    return HD_OK;
}
int MaskState::clear_slots(hd_ctx* c, int n, const int32_t* slots_host, const int* slots_dev, hipStream_t s) {
    if (!unset_slots(faces, c->ws->B, n, slots_host)) return HD_OK;
    MaskScatterP mp{};
    mp.on = on; mp.slots = slots_dev; mp.ll = c->L * c->L;
    hipLaunchKernelGGL(mask_scatter_kernel, dim3(1, n), dim3(64), 0, s, mp);
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}

bool GuideState::active(const hd_ctx* c) const { return on && faces.any(c->ws->B); }
void GuideState::fill(const hd_ctx* c, StepState& st, size_t f0) const {
    st.gd_lp = lp + f0 * 4 * c->L * c->L; st.gd_w = w + f0; st.gd_n = n + f0;
    st.gd_j0 = rows + f0; st.gd_j1 = rows + cap + f0;
}
int GuideState::clear_all(hd_ctx* c, hipStream_t s) {       // weight 0: not guided
    if (faces.count() > 0) HIPCHECK(c, hipMemsetAsync(w, 0, (size_t)cap * sizeof(float), s));
    faces.drop();
    return HD_OK;
}
int GuideState::clear_slots(hd_ctx* c, int n_slots, const int32_t* slots_host, const int* slots_dev, hipStream_t s) {
    if (!unset_slots(faces, c->ws->B, n_slots, slots_host)) return HD_OK;
    GuideScatterP gp{};
    gp.w = w; gp.slots = slots_dev;
    hipLaunchKernelGGL(guide_scatter_kernel, dim3(1, n_slots), dim3(64), 0, s, gp);
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}

bool PreviewState::active(const hd_ctx* c) const { return on && x0 && B == c->ws->B && planes == snaps; }
void PreviewState::fill(const hd_ctx* c, StepState& st, size_t f0) const {
    const size_t per_face = (size_t)4 * c->L * c->L;
    st.pv_x0 = x0 + f0 * per_face; st.pv_snap = snap + f0 * per_face; st.pv_row = row + f0;
    st.pv_every = every; st.pv_snaps = snaps; st.pv_batch = c->ws->B;
}
void PreviewState::free_planes(hd_ctx* c) {
    for (void* p : {(void*)x0, (void*)snap, (void*)row, (void*)slots}) dev_free(c, p);
    x0 = snap = nullptr; row = slots = nullptr; B = 0;
}
// the planes are (re)allocated when the batch or the snapshot count has changed: B is the snapshot-plane stride
int PreviewState::clear_all(hd_ctx* c, hipStream_t s) {
    if (!on) return HD_OK;
    const size_t nB = (size_t)c->ws->B, per_face = (size_t)4 * c->L * c->L, np = (size_t)snaps;
    if (B != c->ws->B || planes != snaps) {
        B = 0;
        const int rc = realloc_buffers(c, {buf_spec(&x0, nB * per_face, false), buf_spec(&snap, (np ? np : 1) * nB * per_face, false),
                                           buf_spec(&row, (1 + np) * nB, false), buf_spec(&slots, nB, false)}, s);
        if (rc) return rc;
        B = c->ws->B; planes = snaps;
    }
    HIPCHECK(c, hipMemsetAsync(x0, 0, nB * per_face * sizeof(float), s));
    if (np) HIPCHECK(c, hipMemsetAsync(snap, 0, np * nB * per_face * sizeof(float), s));
    HIPCHECK(c, hipMemsetAsync(row, 0xff, (1 + np) * nB * sizeof(int), s));      // -1
    return HD_OK;
}
int PreviewState::clear_slots(hd_ctx* c, int n, const int32_t*, const int* slots_dev, hipStream_t s) {
    if (!active(c)) return HD_OK;
    PreviewP pp{};
    pp.x0 = x0; pp.snap = snap; pp.rows = row; pp.slots = slots_dev;
    pp.B = c->ws->B; pp.snaps = snaps; pp.ll4 = 4 * c->L * c->L;
    hipLaunchKernelGGL(preview_reset_kernel, dim3(4, n), dim3(256), 0, s, pp);
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}

// a new batch has no multistep history to resume; a refilled face has none, and hd_sample_rows_multistep(resume = 1) no longer
// continues the whole batch
int HistState::clear_all(hd_ctx*, hipStream_t) { valid = false; faces.drop(); return HD_OK; }
int HistState::clear_slots(hd_ctx* c, int n, const int32_t* slots_host, const int*, hipStream_t) {
    unset_slots(faces, c->ws->B, n, slots_host);
    valid = false;
    return HD_OK;
}

// the common end of every hd_prepare*
static int finish_prepare(hd_ctx* c, hipStream_t s) {
    const int rc = extras_clear_all(c, s);
    if (rc) return rc;
    c->prepared = true;
    return HD_OK;
}

#define HD_NEED_CONDITIONAL(c, what) \
    do { if ((c) && !(c)->conditional) HD_FAIL(c, HD_ERR_INVALID, what ": this context holds the unconditional Denoiser or CoarseRestoration (no priors / identity)"); } while (0)

// Unconditional Denoiser: nothing to condition on -- size the workspace for `batch` faces and build the launch program.
int hd_prepare_unconditional(hd_ctx* c, int batch, void* stream) {
    if (c && (c->cr || c->lpips)) HD_FAIL(c, HD_ERR_INVALID, "hd_prepare_unconditional: this context holds CoarseRestoration or LPIPS");
    if (c && c->conditional) HD_FAIL(c, HD_ERR_INVALID, "hd_prepare_unconditional: this context holds the conditional FusedDenoiser");
    int rc = prepare_common(c, batch);
    if (rc) return rc;
    return finish_prepare(c, reinterpret_cast<hipStream_t>(stream));
}

int hd_prepare(hd_ctx* c, int batch, const float* cr_latent, const float* cr_face, const float* id_emb, void* stream) {
    HD_NEED_CONDITIONAL(c, "hd_prepare");
    int rc = prepare_common(c, batch);
    if (rc) return rc;
    if (!cr_latent || (!cr_face == !id_emb)) HD_FAIL(c, HD_ERR_INVALID, "need cr_latent and exactly one of cr_face / id_emb");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lat_face = (size_t)4 * c->L * c->L;
    for (auto& ch : c->ws->chains) {
        ChainCursor on(c, &ch);
        std::vector<Op> prog;
        add_fpg(c, prog, cr_latent + ch.face0 * lat_face);
        if (cr_face) add_resnet(c, prog, cr_face + (size_t)ch.face0 * 3 * 128 * 128);
        else HIPCHECK(c, hipMemcpyAsync(ch.id_emb, id_emb + (size_t)ch.face0 * 2048, (size_t)ch.B * 2048 * sizeof(float), hipMemcpyDeviceToDevice, s));
        for (int i = 0; i < 5; ++i) add_gates(c, prog, i);
        add_idc_term(c, prog);
        rc = run_ops(c, prog, s, ch.index == 0 ? c->prep_limit : -1);
        ch.prep_program.swap(prog);
        if (rc) return rc;
    }
    return finish_prepare(c, s);
}

int hd_prepare_from_priors(hd_ctx* c, int batch, const float* const priors[5], const float* id_emb, void* stream) {
    HD_NEED_CONDITIONAL(c, "hd_prepare_from_priors");
    int rc = prepare_common(c, batch);
    if (rc) return rc;
    if (!priors || !id_emb) HD_FAIL(c, HD_ERR_INVALID, "priors and id_emb are required");
    for (int i = 0; i < 5; ++i) if (!priors[i]) HD_FAIL(c, HD_ERR_INVALID, "prior %d is NULL", i);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (auto& ch : c->ws->chains) {
        ChainCursor on(c, &ch);
        for (int i = 0; i < 5; ++i) {
            const Level& lv = ch.lv[4 - i];
            const size_t total = (size_t)lv.M * lv.C;          // per chain; faces are contiguous in NCHW too
            hipLaunchKernelGGL(nchw_to_nhwc_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                               priors[i] + (size_t)ch.face0 * lv.C * lv.H * lv.H, ch.prior[i], lv.C, lv.H * lv.H, total);
        }
        HIPCHECK(c, hipGetLastError());
        HIPCHECK(c, hipMemcpyAsync(ch.id_emb, id_emb + (size_t)ch.face0 * 2048, (size_t)ch.B * 2048 * sizeof(float), hipMemcpyDeviceToDevice, s));
        std::vector<Op> prog;
        for (int i = 0; i < 5; ++i) add_gates(c, prog, i);
        add_idc_term(c, prog);
        rc = run_ops(c, prog, s);
        if (rc) return rc;
    }
    return finish_prepare(c, s);
}

int hd_fpg(hd_ctx* c, int batch, const float* cr_latent, float* const priors_out[5], void* stream) {
    HD_NEED_CONDITIONAL(c, "hd_fpg");
    int rc = prepare_common(c, batch);
    if (rc) return rc;
    if (!cr_latent || !priors_out) HD_FAIL(c, HD_ERR_INVALID, "hd_fpg: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lat_face = (size_t)4 * c->L * c->L;
    for (auto& ch : c->ws->chains) {
        ChainCursor on(c, &ch);
        std::vector<Op> prog;
        add_fpg(c, prog, cr_latent + ch.face0 * lat_face);
        rc = run_ops(c, prog, s);
        if (rc) return rc;
        for (int i = 0; i < 5; ++i) {
            if (!priors_out[i]) continue;
            const Level& lv = ch.lv[4 - i];
            const size_t total = (size_t)lv.M * lv.C;
            hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ch.prior[i],
                               priors_out[i] + (size_t)ch.face0 * lv.C * lv.H * lv.H, lv.C, lv.H * lv.H, total);
        }
    }
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}

int hd_idc(hd_ctx* c, int batch, const float* cr_face, float* id_emb_out, void* stream) {
    HD_NEED_CONDITIONAL(c, "hd_idc");
    int rc = prepare_common(c, batch);
    if (rc) return rc;
    if (!cr_face || !id_emb_out) HD_FAIL(c, HD_ERR_INVALID, "hd_idc: bad arguments");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (auto& ch : c->ws->chains) {
        ChainCursor on(c, &ch);
        std::vector<Op> prog;
        add_resnet(c, prog, cr_face + (size_t)ch.face0 * 3 * 128 * 128);
        rc = run_ops(c, prog, s);
        if (rc) return rc;
        HIPCHECK(c, hipMemcpyAsync(id_emb_out + (size_t)ch.face0 * 2048, ch.id_emb, (size_t)ch.B * 2048 * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return HD_OK;
}

int hd_scheduler_step(float* x_inout, const float* eps, const float* coef7, const float* noise, uint64_t seed, int step,
                      int64_t n_elems, void* stream) {
    if (!x_inout || !eps || !coef7 || n_elems <= 0) return HD_ERR_INVALID;
    Coef7 k;
    for (int i = 0; i < 7; ++i) k.c[i] = coef7[i];
    hipLaunchKernelGGL(sched_step_direct_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       x_inout, eps, k, noise, (unsigned long long)seed, step, (long long)n_elems, (float*)nullptr, 0.f);
    return hipGetLastError() == hipSuccess ? HD_OK : HD_ERR_HIP;
}

int hd_scheduler_step_multistep(float* x_inout, const float* eps, const float* coef8, float* x0_hist, const float* noise, uint64_t seed,
                                int step, int64_t n_elems, void* stream) {
    if (!x_inout || !eps || !coef8 || n_elems <= 0) return HD_ERR_INVALID;
    if (!x0_hist && coef8[7] != 0.f) return HD_ERR_INVALID;      // a history term needs the history
    Coef7 k;
    for (int i = 0; i < 7; ++i) k.c[i] = coef8[i];
    hipLaunchKernelGGL(sched_step_direct_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       x_inout, eps, k, noise, (unsigned long long)seed, step, (long long)n_elems, x0_hist, coef8[7]);
    return hipGetLastError() == hipSuccess ? HD_OK : HD_ERR_HIP;
}

int hd_eps(hd_ctx* c, const float* x, const float* timesteps, int n_t, float* eps_out, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    rc = check_xcd(c);
    if (rc) return rc;
    if (!x || !timesteps || !eps_out || (n_t != 1 && n_t != c->ws->B)) HD_FAIL(c, HD_ERR_INVALID, "hd_eps: bad arguments (n_t must be 1 or batch)");
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = ensure_film_rows(c, n_t);
    if (rc) return rc;
    const size_t nlat = (size_t)c->ws->B * 4 * c->L * c->L;
    HIPCHECK(c, hipMemcpyAsync(c->ws->lat, x, nlat * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (auto& ch : c->ws->chains) HIPCHECK(c, hipMemsetAsync(ch.step_state, 0, sizeof(StepState), s));
    c->film_valid = false;                               // rows [0, n_t) are overwritten
    rc = compute_film(c, timesteps, n_t, s);
    if (rc) return rc;
    c->mode = (n_t == 1) ? EvalMode::EpsShared : EvalMode::EpsFaces;
    for (auto& ch : c->ws->chains) {
        rc = run_ops(c, ch.program, s, ch.index == 0 ? c->op_limit : -1);
        if (rc) return rc;
    }
    rc = poison_on_abort(c, c->ws->eps, nlat, s);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpyAsync(eps_out, c->ws->eps, nlat * sizeof(float), hipMemcpyDeviceToDevice, s));
    return HD_OK;
}

// The sampling loop.  Every hd_sample* entry point checks its own arguments, describes the call in a SampleCall (hd_internal.hpp) and runs
// sample_impl: a sequence of steps that each read the descriptor.  What the descriptor leaves NULL stays NULL in StepState, and the kernels
// branch on those pointers: hd_sample (ncoef 7) keeps its [n][7] table and one StepState whose x0_hist is NULL, so its launches and their
// memory traffic are those of a single-step-only build; hd_sample_multistep (ncoef 8) sends c7 to its own [n] table and gives every chain's
// StepState its x0 history.  start_rows (hd_sample_rows*, host [B], already checked): n_iters iterations of the per-face graphs
// (Chain::graph_rows_*), StepState carries the start rows and hist_first = !resume; without them n_iters = n on the graphs of hd_sample.
// face_seeds / first (hd_sample_faces*): StepState also carries the faces' Philox keys and first-order flags (in place of hist_first).
// begin_rows / end_rows (hd_sample_spans): StepState also carries every face's span [begin_f, end_f) of the table -- the face is held from
// row end_f on and its noise counter starts at begin_f.  The table is the concatenation of the members' schedules, so its FiLM table is as
// long as all of them together (0.5 MB per row at latent 16).
// The staging buffer written two calls ago, at least `bytes` large: its copy-done event is the only thing a call ever waits for.  The
// caller fills it, issues its copies on s and ends with stage_submit.
static int stage_acquire(hd_ctx* c, size_t bytes, hd_ctx::Stage** out) {
    auto& sg = c->stage[c->stage_idx ^= 1];
    const size_t need = (bytes + sizeof(float) - 1) / sizeof(float);
    if (sg.pending) { HIPCHECK(c, hipEventSynchronize(sg.ev)); sg.pending = false; }
    if (sg.cap < need) {
        if (sg.host) (void)hipHostFree(sg.host);
        sg.host = nullptr; sg.cap = 0;
        HIPCHECK(c, hipHostMalloc(reinterpret_cast<void**>(&sg.host), need * sizeof(float), hipHostMallocDefault));
        sg.cap = need;
    }
    if (!sg.ev) HIPCHECK(c, hipEventCreateWithFlags(&sg.ev, hipEventDisableTiming));
    *out = &sg;
    return HD_OK;
}
static int stage_submit(hd_ctx* c, hd_ctx::Stage* sg, hipStream_t s) {
    HIPCHECK(c, hipEventRecord(sg->ev, s));
    sg->pending = true;
    return HD_OK;
}
// a slot list of n entries to `dev`: the caller's array is free on return and nothing waits for the stream
static int stage_slots(hd_ctx* c, int* dev, const int32_t* slots, int n, hipStream_t s) {
    hd_ctx::Stage* sg;
    int rc = stage_acquire(c, (size_t)n * sizeof(int32_t), &sg);
    if (rc) return rc;
    memcpy(sg->host, slots, (size_t)n * sizeof(int32_t));
    HIPCHECK(c, hipMemcpyAsync(dev, sg->host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return stage_submit(c, sg, s);
}

static int grow_loop_buffers(hd_ctx* c, const SampleCall& call) {
    const int n = call.n;
    int rc = ensure_film_rows(c, n);
    if (rc) return rc;
    if (n > c->coef_cap) {
        dev_free(c, c->coef_dev);
        rc = dev_alloc(c, &c->coef_dev, (size_t)n * 7);
        if (rc) return rc;
        c->coef_cap = n;
        invalidate_step_graphs(c);                        // every workspace's ending launch captured the old buffer (SchedArgs::coef)
    }
    if (call.start_rows && (size_t)c->ws->B * c->film_total > c->film_pf_cap) {   // the per-face graphs hold this pointer
        dev_free(c, c->film_pf);
        rc = dev_alloc(c, &c->film_pf, (size_t)c->ws->B * c->film_total);
        if (rc) return rc;
        c->film_pf_cap = (size_t)c->ws->B * c->film_total;
        ++c->rows_gen;
    }
    if (call.start_rows && c->ws->B > c->faces_cap) {         // read through StepState and by the gather launch: no graph holds this pointer
        dev_free(c, c->faces_dev);
        c->faces_dev = nullptr; c->faces_cap = 0;
        rc = dev_alloc(c, &c->faces_dev, (size_t)c->ws->B * kFaceArgBytes / sizeof(*c->faces_dev));
        if (rc) return rc;
        c->faces_cap = c->ws->B;
    }
    if (call.ncoef == 8 && n > c->c7_cap) {               // read through StepState: no graph holds this pointer
        dev_free(c, c->c7_dev);
        rc = dev_alloc(c, &c->c7_dev, (size_t)n);
        if (rc) return rc;
        c->c7_cap = n;
    }
    return HD_OK;
}

// Schedule and loop state (step = -1: each chain's intro kernel pre-increments) go through the pinned staging buffer, so the caller's
// host arrays are free on return and nothing here waits for the stream.  Regions, in order: coef [n][7] | timesteps [n] | c7 [n]
// (multistep) | one StepState (single-step, whole batch, no masks, no guidance, no previews) or one per chain | the per-face argument block (per-face calls).
static int stage_loop_state(hd_ctx* c, const SampleCall& call, bool upload_timesteps, hipStream_t s) {
    const int n = call.n;
    const bool ms = call.ncoef == 8, pf = call.start_rows != nullptr;
    const size_t nst = (ms || pf || extras_active(c)) ? c->ws->chains.size() : 1;
    StageCursor cur;
    const size_t coef0 = cur.take((size_t)n * 7 * sizeof(float)), ts0 = cur.take((size_t)n * sizeof(float));
    const size_t c70 = cur.take(ms ? (size_t)n * sizeof(float) : 0), st0 = cur.take(nst * sizeof(StepState));
    const size_t faces0 = cur.take(pf ? (size_t)c->ws->B * kFaceArgBytes : 0);
    hd_ctx::Stage* sg;
    int rc = stage_acquire(c, cur.at, &sg);
    if (rc) return rc;
    char* host = reinterpret_cast<char*>(sg->host);
    float* hcoef = reinterpret_cast<float*>(host + coef0);
    StepState st{};
    st.step = -1; st.n_steps = n; st.noise = call.noise; st.seed = call.seed;
    if (!ms) {
        memcpy(hcoef, call.coef, (size_t)n * 7 * sizeof(float));
    } else {
        float* hc7 = reinterpret_cast<float*>(host + c70);
        for (int i = 0; i < n; ++i) {
            memcpy(hcoef + (size_t)i * 7, call.coef + (size_t)i * 8, 7 * sizeof(float));
            hc7[i] = call.coef[(size_t)i * 8 + 7];
        }
        st.c7 = c->c7_dev;
        HIPCHECK(c, hipMemcpyAsync(c->c7_dev, hc7, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    }
    memcpy(host + ts0, call.timesteps, (size_t)n * sizeof(float));
    if (pf) st.hist_first = call.resume ? 0 : 1;
    const FaceArgs dev = face_args(c->faces_dev, c->ws->B);    // only the arrays the call gave are handed on
    for (size_t k = 0; k < nst; ++k) {
        const size_t f0 = (size_t)c->ws->chains[k].face0;
        if (ms) st.x0_hist = c->ws->chains[k].x0_hist;
        if (pf) st.start_rows = dev.rows + f0;
        if (call.face_seeds) st.face_seeds = dev.seeds + f0;
        if (call.first) st.face_first = dev.first + f0;
        if (call.begin_rows) { st.begin_rows = dev.begins + f0; st.end_rows = dev.ends + f0; }
        each_extra(c, [&](auto& x) { if (x.active(c)) x.fill(c, st, f0); return HD_OK; });
        memcpy(host + st0 + k * sizeof(StepState), &st, sizeof(st));
    }
    if (pf) {                                             // one upload; an array the call did not give is zero and nothing reads it
        const FaceArgs h = face_args(host + faces0, c->ws->B);
        const size_t B = (size_t)c->ws->B;
        memset(host + faces0, 0, B * kFaceArgBytes);
        memcpy(h.rows, call.start_rows, B * sizeof(int32_t));
        if (call.face_seeds) memcpy(h.seeds, call.face_seeds, B * sizeof(uint64_t));
        if (call.first) memcpy(h.first, call.first, B * sizeof(int32_t));
        if (call.begin_rows) { memcpy(h.begins, call.begin_rows, B * sizeof(int32_t)); memcpy(h.ends, call.end_rows, B * sizeof(int32_t)); }
        HIPCHECK(c, hipMemcpyAsync(c->faces_dev, host + faces0, B * kFaceArgBytes, hipMemcpyHostToDevice, s));
    }
    HIPCHECK(c, hipMemcpyAsync(c->coef_dev, hcoef, (size_t)n * 7 * sizeof(float), hipMemcpyHostToDevice, s));
    for (size_t k = 0; k < c->ws->chains.size(); ++k)
        HIPCHECK(c, hipMemcpyAsync(c->ws->chains[k].step_state, host + st0 + (nst > 1 ? k : 0) * sizeof(StepState), sizeof(st), hipMemcpyHostToDevice, s));
    if (upload_timesteps) HIPCHECK(c, hipMemcpyAsync(c->t_dev, host + ts0, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    return stage_submit(c, sg, s);
}

// The FiLM table of the whole schedule (0.5 GB at 1000 steps) is computed once per schedule from t_dev; then the row(s) of the first
// iteration are staged: the ending launch of iteration i stages those of iteration i + 1.
static int film_for_call(hd_ctx* c, const SampleCall& call, bool reuse, hipStream_t s) {
    if (!reuse) {
        c->film_valid = false;
        int rc = compute_film(c, c->t_dev, call.n, s);
        if (rc) return rc;
        if (!c->film_ev) HIPCHECK(c, hipEventCreateWithFlags(&c->film_ev, hipEventDisableTiming));
        HIPCHECK(c, hipEventRecord(c->film_ev, s));
        c->film_sched.assign(call.timesteps, call.timesteps + call.n);
        c->film_valid = true;
    } else {
        HIPCHECK(c, hipStreamWaitEvent(s, c->film_ev, 0));       // no-op on the stream that computed it
    }
    if (call.start_rows) {                                // every face's row r_f (clamped to its last row)
        const FaceArgs dev = face_args(c->faces_dev, c->ws->B);
        hipLaunchKernelGGL(film_rows_gather_kernel, dim3(8, c->ws->B), dim3(256), 0, s, c->film_pf, c->film_table, dev.rows,
                           call.end_rows ? dev.ends : nullptr, call.n, c->film_total);
        HIPCHECK(c, hipGetLastError());
    } else {
        for (auto& ch : c->ws->chains)                      // row 0
            HIPCHECK(c, hipMemcpyAsync(ch.film_cur, c->film_table, (size_t)c->film_total * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return HD_OK;
}

// One graph pair per chain: its launch program + its scheduler update, one step and kGraphSteps steps back to back (fewer graph
// launches).  Faces never interact, so the chains are independent over the whole loop and each graph is replayed on the chain's own
// stream.  pf: the per-face pair (Chain::graph_rows_*), captured in EvalMode::LoopRows like every pair in the mode sample_impl set.
// Nothing is captured while the pair asked for is current.
static int capture_step_graphs(hd_ctx* c, bool pf) {
    bool stale = c->ws->graph_gen != c->graphs_gen || c->ws->graph_film != c->film_table || c->ws->graph_B != c->ws->B;
    if (pf) {
        stale = false;
        for (auto& ch : c->ws->chains) stale |= !ch.graph_rows_exec || ch.rows_gen != c->rows_gen || ch.rows_film != c->film_table;
    }
    if (!stale) return HD_OK;
    c->stage_count = c->face_stage_count = 0;
    for (auto& ch : c->ws->chains) {
        hipGraphExec_t& g1 = pf ? ch.graph_rows_exec : ch.graph_exec;
        hipGraphExec_t& gm = pf ? ch.graph_rows_multi : ch.graph_multi;
        if (g1) { (void)hipGraphExecDestroy(g1); g1 = nullptr; }
        if (gm) { (void)hipGraphExecDestroy(gm); gm = nullptr; }
        for (int multi = 0; multi < 2; ++multi) {
            hipGraph_t graph = nullptr;
            hipError_t e = hipStreamBeginCapture(ch.stream, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                for (int r = 0; r < (multi ? graph_steps() : 1) && e == hipSuccess; ++r)
                    for (size_t k = 0; k < ch.program.size() && e == hipSuccess; ++k) e = ch.program[k].run(ch.stream);
                hipError_t e2 = hipStreamEndCapture(ch.stream, &graph);
                if (e == hipSuccess) e = e2;
            }
            if (e == hipSuccess) e = hipGraphInstantiate(multi ? &gm : &g1, graph, nullptr, nullptr, 0);
            if (e == hipSuccess) ++c->graph_captures;
            if (graph) (void)hipGraphDestroy(graph);
            if (e != hipSuccess) HD_FAIL(c, HD_ERR_HIP, "graph capture/instantiate failed: %s", hipGetErrorString(e));
            if (multi == 0 && &ch == &c->ws->chains[0]) {      // the one-step program of chain 0: what hd_get_option reports
                (pf ? c->rows_stages : c->sample_stages) = c->stage_count;
                if (!pf) c->sample_face_stages = c->face_stage_count;
            }
        }
        if (pf) { ch.rows_gen = c->rows_gen; ch.rows_film = c->film_table; }
    }
    if (!pf) { c->ws->graph_gen = c->graphs_gen; c->ws->graph_film = c->film_table; c->ws->graph_B = c->ws->B; }
    return HD_OK;
}

static int replay_step_graphs(hd_ctx* c, bool pf, int n_iters, hipStream_t s) {
    if (c->profiling) HIPCHECK(c, hipEventRecord(c->ev0, s));
    HIPCHECK(c, hipEventRecord(c->fork_ev, s));
    for (auto& ch : c->ws->chains) HIPCHECK(c, hipStreamWaitEvent(ch.stream, c->fork_ev, 0));
    int i = 0;
    for (; i + graph_steps() <= n_iters; i += graph_steps())
        for (auto& ch : c->ws->chains) HIPCHECK(c, hipGraphLaunch(pf ? ch.graph_rows_multi : ch.graph_multi, ch.stream));
    for (; i < n_iters; ++i)
        for (auto& ch : c->ws->chains) HIPCHECK(c, hipGraphLaunch(pf ? ch.graph_rows_exec : ch.graph_exec, ch.stream));
    for (auto& ch : c->ws->chains) {
        HIPCHECK(c, hipEventRecord(ch.done, ch.stream));
        HIPCHECK(c, hipStreamWaitEvent(s, ch.done, 0));
    }
    if (c->profiling) { HIPCHECK(c, hipEventRecord(c->ev1, s)); c->last_steps = n_iters; }
    return HD_OK;
}

// What a later hd_sample_rows_multistep(resume = 1) may continue, and per face what hd_sample_faces_multistep / hd_sample_spans
// (resume[f] = 1) may: a whole-batch call leaves every face's history (multistep) or none; a multistep per-face call that of every face
// that ran a row.  hist.valid after a rows-multistep call holds regardless of held faces; after a call with per-face flags
// (faces / spans) only when every face has a history.
static void record_history(hd_ctx* c, const SampleCall& call) {
    const bool ms = call.ncoef == 8;
    const int B = c->ws->B;
    FaceSet& hf = c->hist.faces;
    const bool some = ms && call.start_rows;              // only the faces that ran a row gain a history; the others keep what they have
    if (!some || !hf.valid_for(B)) hf.reset(B);
    for (int f = 0; f < B && ms; ++f)
        if (!some || call.start_rows[f] < (call.end_rows ? call.end_rows[f] : call.n)) hf.set(f, true);
    c->hist.valid = ms && (!call.first || hf.all(B));
}

static int sample_impl(hd_ctx* c, float* x_inout, const SampleCall& call, void* stream) {
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool pf = call.start_rows != nullptr;
    const int n_iters = pf ? call.n_iters : call.n;
    const size_t nlat = (size_t)c->ws->B * 4 * c->L * c->L;
    int rc = grow_loop_buffers(c, call);
    if (rc) return rc;
    const bool reuse_film = c->film_valid && c->film_sched.size() == (size_t)call.n &&
                            memcmp(c->film_sched.data(), call.timesteps, (size_t)call.n * sizeof(float)) == 0;
    rc = stage_loop_state(c, call, !reuse_film, s);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpyAsync(c->ws->lat, x_inout, nlat * sizeof(float), hipMemcpyDeviceToDevice, s));
    c->mode = pf ? EvalMode::LoopRows : EvalMode::LoopShared;
    rc = film_for_call(c, call, reuse_film, s);
    if (!rc) rc = capture_step_graphs(c, pf);
    if (!rc) rc = replay_step_graphs(c, pf, n_iters, s);
    if (rc) return rc;
    record_history(c, call);
    rc = poison_on_abort(c, c->ws->lat, nlat, s);
    if (rc) return rc;
    HIPCHECK(c, hipMemcpyAsync(x_inout, c->ws->lat, nlat * sizeof(float), hipMemcpyDeviceToDevice, s));
    return HD_OK;
}

// What every sampling entry point opens with: the context is ready and no stage of an earlier call gave up, the latents and the table
// are there (args_ok: the entry point's other required arguments are, too); then the table goes into the descriptor.
static int sample_enter(hd_ctx* c, const char* fn, const float* x, const hd_schedule* sched, int ncoef, bool args_ok, const float* noise,
                        uint64_t seed, SampleCall& call) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    rc = check_xcd(c);
    if (rc) return rc;
    if (!x || !sched || sched->n_steps <= 0 || !sched->timesteps || !sched->coef || !args_ok) HD_FAIL(c, HD_ERR_INVALID, "%s: bad arguments", fn);
    call.fn = fn;
    call.n = sched->n_steps; call.timesteps = sched->timesteps; call.coef = sched->coef;
    call.ncoef = ncoef;
    call.noise = noise; call.seed = seed;
    return HD_OK;
}

// hd_schedule_ms is hd_schedule with 8 coefficients per row
static const hd_schedule* as_rows_of_8(const hd_schedule_ms* s) { return reinterpret_cast<const hd_schedule*>(s); }
static_assert(sizeof(hd_schedule) == sizeof(hd_schedule_ms), "the two schedule structs share one layout");

// start rows in [0, n], n_iters in [1, n - min r_f]; then they go into the descriptor
static int check_rows(hd_ctx* c, SampleCall& call, const int32_t* rows, int n_iters) {
    const int n = call.n;
    int rmin = n;
    for (int f = 0; f < c->ws->B; ++f) {
        if (rows[f] < 0 || rows[f] > n) HD_FAIL(c, HD_ERR_INVALID, "%s: start_rows[%d] = %d outside [0, %d]", call.fn, f, rows[f], n);
        if (rows[f] < rmin) rmin = rows[f];
    }
    if (n_iters < 1 || n_iters > n - rmin) HD_FAIL(c, HD_ERR_INVALID, "%s: n_iters = %d outside [1, %d]", call.fn, n_iters, n - rmin);
    call.start_rows = rows; call.n_iters = n_iters;
    return HD_OK;
}

// resume[f] of hd_sample_faces_multistep / hd_sample_spans: 0 or 1, and 1 only for a face that has a history; first_f = !resume_f
static int check_face_resume(hd_ctx* c, const char* fn, int f, int32_t resume_f, int32_t* first_f) {
    if (resume_f != 0 && resume_f != 1) HD_FAIL(c, HD_ERR_INVALID, "%s: resume[%d] = %d is not 0 or 1", fn, f, resume_f);
    if (resume_f && !(c->hist.faces.valid_for(c->ws->B) && c->hist.faces.get(f)))
        HD_FAIL(c, HD_ERR_INVALID, "%s: resume[%d] = 1 but face %d has no multistep history (no multistep row since "
                                   "hd_prepare*, hd_prepare_slots refilled it, or a single-step call in between)", fn, f, f);
    *first_f = resume_f ? 0 : 1;
    return HD_OK;
}

int hd_sample(hd_ctx* c, float* x_inout, const hd_schedule* sched, const float* noise, uint64_t seed, void* stream) {
    SampleCall call;
    int rc = sample_enter(c, "hd_sample", x_inout, sched, 7, true, noise, seed, call);
    return rc ? rc : sample_impl(c, x_inout, call, stream);
}

int hd_sample_multistep(hd_ctx* c, float* x_inout, const hd_schedule_ms* sched, const float* noise, uint64_t seed, void* stream) {
    SampleCall call;
    int rc = sample_enter(c, "hd_sample_multistep", x_inout, as_rows_of_8(sched), 8, true, noise, seed, call);
    if (rc) return rc;
    // the first step has no previous x0: the history of the call starts there (never inherited from an earlier call)
    if (sched->coef[7] != 0.f) HD_FAIL(c, HD_ERR_INVALID, "hd_sample_multistep: row 0 must have c7 == 0 (no history before the first step)");
    return sample_impl(c, x_inout, call, stream);
}

int hd_sample_rows(hd_ctx* c, float* x_inout, const hd_schedule* sched, const int32_t* start_rows, int n_iters, const float* noise,
                   uint64_t seed, void* stream) {
    SampleCall call;
    int rc = sample_enter(c, "hd_sample_rows", x_inout, sched, 7, start_rows != nullptr, noise, seed, call);
    if (!rc) rc = check_rows(c, call, start_rows, n_iters);
    if (rc) return rc;
    return sample_impl(c, x_inout, call, stream);
}

int hd_sample_rows_multistep(hd_ctx* c, float* x_inout, const hd_schedule_ms* sched, const int32_t* start_rows, int n_iters, int resume,
                             const float* noise, uint64_t seed, void* stream) {
    SampleCall call;
    int rc = sample_enter(c, "hd_sample_rows_multistep", x_inout, as_rows_of_8(sched), 8, start_rows && (resume == 0 || resume == 1), noise, seed, call);
    if (!rc) rc = check_rows(c, call, start_rows, n_iters);
    if (rc) return rc;
    if (resume && !(c->hist.valid && c->hist.faces.valid_for(c->ws->B)))
        HD_FAIL(c, HD_ERR_INVALID, "hd_sample_rows_multistep: resume = 1 but no multistep history of this batch (no earlier multistep call, "
                                   "hd_prepare since, another batch size or a single-step call in between)");
    call.resume = resume;
    return sample_impl(c, x_inout, call, stream);
}

int hd_sample_faces(hd_ctx* c, float* x_inout, const hd_schedule* sched, const int32_t* start_rows, int n_iters, const uint64_t* face_seeds,
                    const float* noise, uint64_t seed, void* stream) {
    SampleCall call;
    int rc = sample_enter(c, "hd_sample_faces", x_inout, sched, 7, start_rows != nullptr, noise, seed, call);
    if (!rc) rc = check_rows(c, call, start_rows, n_iters);
    if (rc) return rc;
    call.face_seeds = face_seeds;
    return sample_impl(c, x_inout, call, stream);
}

int hd_sample_faces_multistep(hd_ctx* c, float* x_inout, const hd_schedule_ms* sched, const int32_t* start_rows, int n_iters,
                              const int32_t* resume, const uint64_t* face_seeds, const float* noise, uint64_t seed, void* stream) {
    SampleCall call;
    int rc = sample_enter(c, "hd_sample_faces_multistep", x_inout, as_rows_of_8(sched), 8, start_rows && resume, noise, seed, call);
    if (!rc) rc = check_rows(c, call, start_rows, n_iters);
    if (rc) return rc;
    std::vector<int32_t> first((size_t)c->ws->B);
    for (int f = 0; f < c->ws->B; ++f) {
        rc = check_face_resume(c, call.fn, f, resume[f], &first[f]);
        if (rc) return rc;
    }
    call.face_seeds = face_seeds; call.first = first.data();
    return sample_impl(c, x_inout, call, stream);
}

// Per-request schedules: `table` is the concatenation of several schedules and face f runs rows start_f, start_f + 1, .. of its own span
// [begin_f, end_f).  Everything else is hd_sample_faces_multistep (a 7-column schedule is the same rows with c7 = 0).
int hd_sample_spans(hd_ctx* c, float* x_inout, const hd_schedule_ms* table, const int32_t* begin_rows, const int32_t* end_rows,
                    const int32_t* start_rows, int n_iters, const int32_t* resume, const uint64_t* face_seeds, const float* noise,
                    uint64_t seed, void* stream) {
    SampleCall call;
    int rc = sample_enter(c, "hd_sample_spans", x_inout, as_rows_of_8(table), 8, begin_rows && end_rows && start_rows && resume, noise, seed, call);
    if (rc) return rc;
    const int n = call.n;
    std::vector<int32_t> first((size_t)c->ws->B);
    int longest = 0;
    for (int f = 0; f < c->ws->B; ++f) {
        const int b = begin_rows[f], e = end_rows[f], r = start_rows[f];
        if (!(0 <= b && b <= r && r <= e && e <= n))
            HD_FAIL(c, HD_ERR_INVALID, "hd_sample_spans: face %d: need 0 <= begin (%d) <= start (%d) <= end (%d) <= n_steps (%d)", f, b, r, e, n);
        if (b < n && table->coef[(size_t)b * 8 + 7] != 0.f)
            HD_FAIL(c, HD_ERR_INVALID, "hd_sample_spans: face %d: row %d begins its schedule and must have c7 == 0 (no history before it)", f, b);
        if (resume[f] == 1 && r == b)
            HD_FAIL(c, HD_ERR_INVALID, "hd_sample_spans: resume[%d] = 1 but face %d starts at its begin row %d (nothing to resume)", f, f, b);
        rc = check_face_resume(c, call.fn, f, resume[f], &first[f]);
        if (rc) return rc;
        if (e - r > longest) longest = e - r;
    }
    if (n_iters < 1 || n_iters > longest) HD_FAIL(c, HD_ERR_INVALID, "hd_sample_spans: n_iters = %d outside [1, %d]", n_iters, longest);
    call.start_rows = start_rows; call.n_iters = n_iters;
    call.begin_rows = begin_rows; call.end_rows = end_rows;
    call.face_seeds = face_seeds; call.first = first.data();
    return sample_impl(c, x_inout, call, stream);
}

// Continuous batching: hd_prepare_slots, hd_pool_prepare and hd_pool_commit are made of the same four pieces.
// check_index_list: a host list `what` of n indices in [0, limit), distinct where asked for.
static int check_index_list(hd_ctx* c, const char* fn, const char* what, const int32_t* v, int n, int limit, bool distinct) {
    std::vector<char> seen(distinct ? (size_t)limit : 0, 0);
    for (int j = 0; j < n; ++j) {
        if (v[j] < 0 || v[j] >= limit) HD_FAIL(c, HD_ERR_INVALID, "%s: %s[%d] = %d outside [0, %d)", fn, what, j, v[j], limit);
        if (!distinct) continue;
        if (seen[v[j]]) HD_FAIL(c, HD_ERR_INVALID, "%s: %s holds %d twice", fn, what, v[j]);
        seen[v[j]] = 1;
    }
    return HD_OK;
}
// The index lists of a call to ws->slots_dev in one upload: a [n], then b [n] (b may be NULL).  The caller's arrays are free on return.
static int stage_index_lists(hd_ctx* c, const int32_t* a, const int32_t* b, int n, hipStream_t s) {
    if (!c->ws->slots_dev) {
        const int rc = ws_alloc(c, &c->ws->slots_dev, (size_t)2 * c->ws->B);
        if (rc) return rc;
    }
    if (!b) return stage_slots(c, c->ws->slots_dev, a, n, s);
    std::vector<int32_t> both((size_t)2 * n);
    memcpy(both.data(), a, (size_t)n * sizeof(int32_t));
    memcpy(both.data() + n, b, (size_t)n * sizeof(int32_t));
    return stage_slots(c, c->ws->slots_dev, both.data(), 2 * n, s);
}
// The conditioning prologue (FPG, ResNet-50 or the given embedding, HCA gates, idc_conv) of n faces at batch n on the workspace's
// private staging chain -- the same launches hd_prepare issues for a batch of n, so the staging chain then holds bit for bit the
// conditioning hd_prepare(n) computes.  Nothing of the batch's chains is read or written.
static int stage_prologue(hd_ctx* c, int n, const float* cr_latent, const float* cr_face, const float* id_emb, hipStream_t s) {
    Chain& sc = c->ws->slot_stage;
    int rc;
    if (!c->ws->slot_stage_ok) {                               // first refill of this workspace: its buffers join the workspace's allocations
        sc = Chain();
        sc.index = -1; sc.B = c->ws->B; sc.face0 = 0;          // index -1: no introspection names (those stay on chain 0)
        rc = alloc_chain(c, sc);
        if (rc) { destroy_chain_queue(sc); return rc; }
        c->ws->slot_stage_ok = true;
    }
    // the staging chain at batch n: the level geometry of a batch of n faces (its buffers hold B)
    sc.B = n;
    for (int l = 0; l < 5; ++l) sc.lv[l].M = n * sc.lv[l].H * sc.lv[l].H;
    std::vector<Op> prog;
    {
        ChainCursor on(c, &sc);
        add_fpg(c, prog, cr_latent);
        if (cr_face) add_resnet(c, prog, cr_face);
        for (int i = 0; i < 5; ++i) add_gates(c, prog, i);
        add_idc_term(c, prog);
    }
    if (!cr_face) HIPCHECK(c, hipMemcpyAsync(sc.id_emb, id_emb, (size_t)n * 2048 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return run_ops(c, prog, s);
}
// The kSlotBufs conditioning buffers of a chain in CondCopyP order, and their per-face sizes (they depend on L only).
static void cond_buffers(const Chain& ch, float* out[kSlotBufs]) {
    int b = 0;
    for (int i = 0; i < 5; ++i) { out[b++] = ch.prior[i]; out[b++] = ch.gate_c[i]; out[b++] = ch.gate_s[i]; }
    out[b++] = ch.idc_term; out[b++] = ch.id_emb;
}
static void cond_sizes(const hd_ctx* c, int sz[kSlotBufs]) {
    int b = 0;
    for (int i = 0; i < 5; ++i) {
        const int C = WIDTH << (4 - i), H = c->L >> (4 - i);    // prior i belongs to level 4 - i (coarsest first)
        sz[b++] = H * H * C; sz[b++] = C; sz[b++] = H * H;      // prior i (NHWC), w_c, w_s per face
    }
    sz[b++] = 2048 * c->S * c->S; sz[b++] = 2048;
}
enum class CondEnd { Staging, Pool, Slots };
// One cond_copy_kernel launch for the n faces of a call: from the staging chain (face j) or the pool (entry src_idx[j]) to the pool
// (entry dst_idx[j]) or the batch's slots (slot dst_idx[j]); the lists are on the device already (stage_index_lists).
static int copy_conditioning(hd_ctx* c, int n, CondEnd from, const int* src_idx, CondEnd to, const int* dst_idx, hipStream_t s) {
    CondCopyP p{};
    cond_sizes(c, p.sz);
    float* bufs[kSlotBufs];
    if (from == CondEnd::Staging) cond_buffers(c->ws->slot_stage, bufs);
    for (int b = 0; b < kSlotBufs; ++b) p.src[b] = from == CondEnd::Staging ? bufs[b] : c->pool_buf[b];
    if (to == CondEnd::Pool) {
        for (int b = 0; b < kSlotBufs; ++b) p.dst[0][b] = c->pool_buf[b];
        p.faces_per_chain = 0;
    } else {
        for (size_t k = 0; k < c->ws->chains.size(); ++k) {
            cond_buffers(c->ws->chains[k], bufs);
            for (int b = 0; b < kSlotBufs; ++b) p.dst[k][b] = bufs[b];
        }
        p.faces_per_chain = c->ws->chains[0].B;
    }
    p.src_idx = src_idx; p.dst_idx = dst_idx;
    hipLaunchKernelGGL(cond_copy_kernel, dim3(32, n, kSlotBufs), dim3(256), 0, s, p);
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}
// The checks the three entry points share: a conditional context with a prepared batch (and, for the pool calls, a pool).
static int slots_enter(hd_ctx* c, const char* fn, bool need_pool) {
    if (!c) return HD_ERR_INVALID;
    if (c->cr || c->vae || !c->conditional)
        HD_FAIL(c, HD_ERR_INVALID, "%s: this context holds the unconditional Denoiser, CoarseRestoration or the VAE (no conditioning)", fn);
    const int rc = check_ready(c, true);
    if (rc) return rc;
    if (need_pool && c->pool_cap == 0) HD_FAIL(c, HD_ERR_NOT_READY, "%s: no pool is configured (hd_pool_config)", fn);
    return HD_OK;
}

// Replace the conditioning of n slots.  The prologue runs at batch n on the workspace's private staging chain, so the n faces'
// conditioning is bit for bit that of hd_prepare(n), and cond_copy_kernel copies it straight into the slots.  Nothing of the batch's
// chains is rebuilt, parked or recaptured; only the refilled slots' buffers are written.
int hd_prepare_slots(hd_ctx* c, int n, const int32_t* slots, const float* cr_latent, const float* cr_face, const float* id_emb, void* stream) {
    int rc = slots_enter(c, "hd_prepare_slots", false);
    if (rc) return rc;
    if (n < 1 || n > c->ws->B) HD_FAIL(c, HD_ERR_INVALID, "hd_prepare_slots: n = %d outside [1, %d]", n, c->ws->B);
    if (!slots || !cr_latent || (!cr_face == !id_emb))
        HD_FAIL(c, HD_ERR_INVALID, "hd_prepare_slots: need slots, cr_latent and exactly one of cr_face / id_emb");
    rc = check_index_list(c, "hd_prepare_slots", "slots", slots, n, c->ws->B, true);
    if (rc) return rc;
    if (c->ws->chains.size() > (size_t)kSlotChains) HD_FAIL(c, HD_ERR_INVALID, "hd_prepare_slots: more than %d chains", kSlotChains);
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = stage_prologue(c, n, cr_latent, cr_face, id_emb, s);
    if (!rc) rc = stage_index_lists(c, slots, nullptr, n, s);
    if (!rc) rc = copy_conditioning(c, n, CondEnd::Staging, nullptr, CondEnd::Slots, c->ws->slots_dev, s);
    if (!rc) rc = extras_clear_slots(c, n, slots, s);
    return rc;
}

// The conditioning pool: `capacity` entries of one face's conditioning each (0: none).  Every entry is invalid afterwards.
int hd_pool_config(hd_ctx* c, int capacity) {
    if (!c) return HD_ERR_INVALID;
    if (c->cr || c->vae || !c->conditional)
        HD_FAIL(c, HD_ERR_INVALID, "hd_pool_config: this context holds the unconditional Denoiser, CoarseRestoration or the VAE (no conditioning)");
    if (capacity < 0 || capacity > 4096) HD_FAIL(c, HD_ERR_INVALID, "hd_pool_config: capacity = %d outside [0, 4096]", capacity);
    HIPCHECK(c, hipSetDevice(c->device));
    if (c->pool_dev) {                                     // copies that read or write the old pool may still be in flight
        HIPCHECK(c, hipDeviceSynchronize());
        dev_free(c, c->pool_dev);
    }
    c->pool_dev = nullptr; c->pool_cap = 0; c->pool_ok.clear();
    for (int b = 0; b < kSlotBufs; ++b) c->pool_buf[b] = nullptr;
    if (capacity == 0) return HD_OK;
    cond_sizes(c, c->pool_sz);
    size_t off[kSlotBufs], total = 0;
    for (int b = 0; b < kSlotBufs; ++b) { off[b] = total; total += ((size_t)capacity * c->pool_sz[b] + 3) / 4 * 4; }   // every buffer starts 16-byte aligned
    const int rc = dev_alloc(c, &c->pool_dev, total);
    if (rc) { c->pool_dev = nullptr; return rc; }
    for (int b = 0; b < kSlotBufs; ++b) c->pool_buf[b] = c->pool_dev + off[b];
    c->pool_cap = capacity;
    c->pool_ok.assign((size_t)capacity, 0);
    return HD_OK;
}

// The prologue of hd_prepare_slots for n faces, kept: face j goes to pool entry entries[j] instead of a slot.  The running batch is not
// touched -- no slot buffer, mask, guidance, preview or history flag -- so a loop split around this call gives the bits it gives without it.
int hd_pool_prepare(hd_ctx* c, int n, const int32_t* entries, const float* cr_latent, const float* cr_face, const float* id_emb, void* stream) {
    int rc = slots_enter(c, "hd_pool_prepare", true);
    if (rc) return rc;
    const int most = c->ws->B < c->pool_cap ? c->ws->B : c->pool_cap;
    if (n < 1 || n > most) HD_FAIL(c, HD_ERR_INVALID, "hd_pool_prepare: n = %d outside [1, %d] (the batch and the pool's capacity)", n, most);
    if (!entries || !cr_latent || (!cr_face == !id_emb))
        HD_FAIL(c, HD_ERR_INVALID, "hd_pool_prepare: need entries, cr_latent and exactly one of cr_face / id_emb");
    rc = check_index_list(c, "hd_pool_prepare", "entries", entries, n, c->pool_cap, true);
    if (rc) return rc;
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = stage_prologue(c, n, cr_latent, cr_face, id_emb, s);
    if (!rc) rc = stage_index_lists(c, entries, nullptr, n, s);
    if (!rc) rc = copy_conditioning(c, n, CondEnd::Staging, nullptr, CondEnd::Pool, c->ws->slots_dev, s);
    if (rc) return rc;
    for (int j = 0; j < n; ++j) c->pool_ok[entries[j]] = 1;
    return HD_OK;
}

// The second half of hd_prepare_slots: slot slots[j] gets a copy of pool entry entries[j] and loses what a refilled slot loses.
int hd_pool_commit(hd_ctx* c, int n, const int32_t* slots, const int32_t* entries, void* stream) {
    int rc = slots_enter(c, "hd_pool_commit", true);
    if (rc) return rc;
    if (n < 1 || n > c->ws->B) HD_FAIL(c, HD_ERR_INVALID, "hd_pool_commit: n = %d outside [1, %d]", n, c->ws->B);
    if (!slots || !entries) HD_FAIL(c, HD_ERR_INVALID, "hd_pool_commit: need slots and entries");
    rc = check_index_list(c, "hd_pool_commit", "slots", slots, n, c->ws->B, true);
    if (!rc) rc = check_index_list(c, "hd_pool_commit", "entries", entries, n, c->pool_cap, false);
    if (rc) return rc;
    for (int j = 0; j < n; ++j)
        if (!c->pool_ok[entries[j]]) HD_FAIL(c, HD_ERR_INVALID, "hd_pool_commit: entries[%d] = %d was never prepared (hd_pool_prepare)", j, entries[j]);
    if (c->ws->chains.size() > (size_t)kSlotChains) HD_FAIL(c, HD_ERR_INVALID, "hd_pool_commit: more than %d chains", kSlotChains);
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = stage_index_lists(c, slots, entries, n, s);
    if (!rc) rc = copy_conditioning(c, n, CondEnd::Pool, c->ws->slots_dev + n, CondEnd::Slots, c->ws->slots_dev, s);
    if (!rc) rc = extras_clear_slots(c, n, slots, s);
    return rc;
}

// What the per-face calls open with (hd_mask_faces, hd_guide_faces, hd_preview_read; the two config calls: loop_ctx_enter alone): a
// context with a sampling loop and a prepared batch (not-ready comes before any argument error), n faces of it, and either no slot
// list (the whole batch, in order) or n distinct slots.
static int loop_ctx_enter(hd_ctx* c, const char* fn) {
    if (!c) return HD_ERR_INVALID;
    if (c->cr || c->vae || c->lpips) HD_FAIL(c, HD_ERR_INVALID, "%s: this context holds CoarseRestoration, the VAE or LPIPS (no sampling loop)", fn);
    return HD_OK;
}
static int faces_enter(hd_ctx* c, const char* fn, int n, const int32_t* slots) {
    int rc = loop_ctx_enter(c, fn);
    if (!rc) rc = check_ready(c, true);
    if (rc) return rc;
    if (n < 1 || n > c->ws->B) HD_FAIL(c, HD_ERR_INVALID, "%s: n = %d outside [1, %d]", fn, n, c->ws->B);
    if (!slots && n != c->ws->B) HD_FAIL(c, HD_ERR_INVALID, "%s: slots == NULL needs n == batch (%d), got %d", fn, c->ws->B, n);
    return slots ? check_index_list(c, fn, "slots", slots, n, c->ws->B, true) : HD_OK;
}

// Give n faces of the prepared batch a mask, the known latent and its noise (or take their masks away: all three NULL).  The tensors are
// copied in stream order into buffers of the context that the step kernels reach through StepState: no launch program is rebuilt and no
// graph recaptured, and while no face is masked the loop's launches read nothing of this.
int hd_mask_faces(hd_ctx* c, int n, const int32_t* slots, const float* mask, const float* known, const float* known_noise, void* stream) {
    int rc = faces_enter(c, "hd_mask_faces", n, slots);
    if (rc) return rc;
    if ((!mask != !known) || (!mask != !known_noise))
        HD_FAIL(c, HD_ERR_INVALID, "hd_mask_faces: give mask, known and known_noise together, or none of them (clear)");
    MaskState& m = c->mask;
    const size_t B = (size_t)c->ws->B, ll = (size_t)c->L * c->L;
    if (!m.faces.valid_for(c->ws->B)) m.faces.reset(c->ws->B);
    if (!mask && m.faces.count() == 0) return HD_OK;       // nothing to clear
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (c->ws->B > m.cap) {                                // a larger batch than ever masked: hd_prepare* has cleared every mask since
        m.cap = 0;
        rc = realloc_buffers(c, {buf_spec(&m.dmask, B * ll, true), buf_spec(&m.dknown, B * 4 * ll, true), buf_spec(&m.dnoise, B * 4 * ll, true),
                                 buf_spec(&m.on, B, true), buf_spec(&m.slots, B, false)}, s);
        if (rc) return rc;
        m.cap = c->ws->B;
    }
    if (slots) {
        rc = stage_slots(c, m.slots, slots, n, s);
        if (rc) return rc;
    }
    MaskScatterP p{};
    p.mask = mask; p.known = known; p.noise = known_noise;
    p.dmask = m.dmask; p.dknown = m.dknown; p.dnoise = m.dnoise;
    p.on = m.on; p.slots = slots ? m.slots : nullptr; p.ll = (int)ll;
    hipLaunchKernelGGL(mask_scatter_kernel, dim3(mask ? 4 : 1, n), dim3(256), 0, s, p);
    HIPCHECK(c, hipGetLastError());
    for (int j = 0; j < n; ++j) m.faces.set(slots ? slots[j] : j, mask != nullptr);
    return HD_OK;
}

// Low-pass fidelity guidance.  The switch decides whether the captured step ends with guided_update_kernel: flipping it makes the step
// graphs stale (one recapture at the next loop), and with it off no launch, graph or bit differs from a context that never had it on.
int hd_guide_config(hd_ctx* c, int on) {
    int rc = loop_ctx_enter(c, "hd_guide_config");
    if (rc) return rc;
    if (on != 0 && on != 1) HD_FAIL(c, HD_ERR_INVALID, "hd_guide_config: on = %d is not 0 or 1", on);
    if (c->guide.on == (on != 0)) return HD_OK;
    if (!on && c->guide.faces.count() > 0) {               // switching off clears every face (the weights in stream order of the null stream)
        HIPCHECK(c, hipSetDevice(c->device));
        HIPCHECK(c, hipDeviceSynchronize());               // a loop in flight may still read them
        rc = c->guide.clear_all(c, nullptr);
        if (rc) return rc;
        HIPCHECK(c, hipStreamSynchronize(nullptr));
    }
    c->guide.faces.drop();
    c->guide.on = on != 0;
    invalidate_step_graphs(c);                             // the ending op launches one kernel more, or one fewer
    return HD_OK;
}

// Guide n faces of the prepared batch towards LP_N of a target (or stop guiding them: target NULL).  LP_N(target) is computed here, once,
// in stream order, into a buffer of the context that the step kernels reach through StepState, with the faces' weights, block sizes and
// row windows: no launch program is rebuilt and no graph recaptured by setting, changing or clearing faces.
int hd_guide_faces(hd_ctx* c, int n, const int32_t* slots, const float* target, const float* weight, const int32_t* scale,
                   const int32_t* row_from, const int32_t* row_to, void* stream) {
    int rc = faces_enter(c, "hd_guide_faces", n, slots);
    if (rc) return rc;
    GuideState& g = c->guide;
    if (target) {
        if (!g.on) HD_FAIL(c, HD_ERR_INVALID, "hd_guide_faces: guidance is switched off (hd_guide_config(ctx, 1) first)");
        if (!weight || !scale) HD_FAIL(c, HD_ERR_INVALID, "hd_guide_faces: a target needs weight and scale");
        if (!row_from != !row_to) HD_FAIL(c, HD_ERR_INVALID, "hd_guide_faces: give row_from and row_to together, or neither (all rows)");
        if (c->L > kGuideMaxL) HD_FAIL(c, HD_ERR_INVALID, "hd_guide_faces: latent %d is larger than %d", c->L, kGuideMaxL);
        for (int j = 0; j < n; ++j) {
            if (!(weight[j] > 0.f && weight[j] <= 1.f)) HD_FAIL(c, HD_ERR_INVALID, "hd_guide_faces: weight[%d] = %g outside (0, 1]", j, (double)weight[j]);
            if (scale[j] < 1 || scale[j] > c->L || c->L % scale[j] != 0)
                HD_FAIL(c, HD_ERR_INVALID, "hd_guide_faces: scale[%d] = %d does not divide the latent size %d", j, scale[j], c->L);
            if (row_from && !(0 <= row_from[j] && row_from[j] < row_to[j]))
                HD_FAIL(c, HD_ERR_INVALID, "hd_guide_faces: rows [%d, %d) of face %d: need 0 <= row_from < row_to", row_from[j], row_to[j], j);
        }
    }
    if (!g.faces.valid_for(c->ws->B)) g.faces.reset(c->ws->B);
    if (!target && g.faces.count() == 0) return HD_OK;     // nothing to clear
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t B = (size_t)c->ws->B, ll = (size_t)c->L * c->L;
    if (c->ws->B > g.cap) {                                // a larger batch than ever guided: hd_prepare* has cleared every face since
        g.cap = 0;
        rc = realloc_buffers(c, {buf_spec(&g.lp, B * 4 * ll, true), buf_spec(&g.w, B, true), buf_spec(&g.n, B, true),
                                 buf_spec(&g.rows, 2 * B, true), buf_spec(&g.args, 5 * B, false)}, s);
        if (rc) return rc;
        g.cap = c->ws->B;
    }
    // the call's host arrays through the pinned staging buffer: slots | weight | scale | row_from | row_to, [n] each
    {
        hd_ctx::Stage* sg;
        rc = stage_acquire(c, (size_t)5 * n * sizeof(int32_t), &sg);
        if (rc) return rc;
        int32_t* h = reinterpret_cast<int32_t*>(sg->host);
        for (int j = 0; j < n; ++j) {
            h[j] = slots ? slots[j] : j;
            const float w = target ? weight[j] : 0.f;
            memcpy(&h[n + j], &w, sizeof(float));
            h[2 * n + j] = target ? scale[j] : 1;
            h[3 * n + j] = (target && row_from) ? row_from[j] : 0;
            h[4 * n + j] = (target && row_from) ? row_to[j] : 0x7fffffff;
        }
        HIPCHECK(c, hipMemcpyAsync(g.args, h, (size_t)5 * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        rc = stage_submit(c, sg, s);
        if (rc) return rc;
    }
    GuideScatterP p{};
    p.target = target; p.lp = g.lp; p.w = g.w; p.n = g.n;
    p.j0 = g.rows; p.j1 = g.rows + g.cap;
    p.slots = g.args; p.weight = reinterpret_cast<const float*>(g.args + n);
    p.scale = g.args + 2 * n; p.row_from = g.args + 3 * n; p.row_to = g.args + 4 * n; p.L = c->L;
    hipLaunchKernelGGL(guide_scatter_kernel, dim3(target ? 4 : 1, n), dim3(256), target ? guide_lds_bytes(c->L) : 0, s, p);
    HIPCHECK(c, hipGetLastError());
    for (int j = 0; j < n; ++j) g.faces.set(slots ? slots[j] : j, target != nullptr);
    return HD_OK;
}

// Progress previews: the denoised estimate of the row a face last ran (and every pv_every-th row of its schedule) as an output of the step
// kernels.  The planes belong to the context and are reached through StepState, like the masks: switching them on or off rebuilds no
// launch program and recaptures no graph, and while they are off the loop's launches read and write nothing of this.
int hd_preview_config(hd_ctx* c, int on, int every, int snapshots) {
    int rc = loop_ctx_enter(c, "hd_preview_config");
    if (rc) return rc;
    if (on != 0 && on != 1) HD_FAIL(c, HD_ERR_INVALID, "hd_preview_config: on = %d is not 0 or 1", on);
    if (every < 1) HD_FAIL(c, HD_ERR_INVALID, "hd_preview_config: every = %d must be >= 1", every);
    if (snapshots < 0 || snapshots > 64) HD_FAIL(c, HD_ERR_INVALID, "hd_preview_config: snapshots = %d outside [0, 64]", snapshots);
    HIPCHECK(c, hipSetDevice(c->device));
    PreviewState& pv = c->preview;
    pv.on = on != 0; pv.every = every; pv.snaps = snapshots;
    if (!on) {
        if (pv.x0) HIPCHECK(c, hipDeviceSynchronize());            // a loop in flight may still write them
        pv.free_planes(c);
        return HD_OK;
    }
    if (!c->finalized || !c->prepared) return HD_OK;         // allocated by the next hd_prepare*
    HIPCHECK(c, hipDeviceSynchronize());
    rc = pv.clear_all(c, nullptr);
    if (rc) return rc;
    HIPCHECK(c, hipStreamSynchronize(nullptr));              // the chains' queues do not wait for the null stream
    return HD_OK;
}

int hd_preview_read(hd_ctx* c, int n, const int32_t* slots, int snapshot, float* x0_out, int32_t* rows_out, void* stream) {
    int rc = faces_enter(c, "hd_preview_read", n, slots);
    if (rc) return rc;
    const PreviewState& pv = c->preview;
    if (!pv.active(c)) HD_FAIL(c, HD_ERR_NOT_READY, "hd_preview_read: previews are off (hd_preview_config)");
    if (!x0_out) HD_FAIL(c, HD_ERR_INVALID, "hd_preview_read: x0_out is NULL");
    if (snapshot < -1 || snapshot >= pv.snaps)
        HD_FAIL(c, HD_ERR_INVALID, "hd_preview_read: snapshot = %d outside [-1, %d)", snapshot, pv.snaps);
    HIPCHECK(c, hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (slots) {
        rc = stage_slots(c, pv.slots, slots, n, s);
        if (rc) return rc;
    }
    const size_t per_face = (size_t)4 * c->L * c->L;
    PreviewReadP p{};
    p.plane = snapshot < 0 ? pv.x0 : pv.snap + (size_t)snapshot * c->ws->B * per_face;
    p.rows = pv.row + (size_t)(1 + snapshot) * c->ws->B;
    p.slots = slots ? pv.slots : nullptr; p.out = x0_out; p.rows_out = rows_out; p.ll4 = (int)per_face;
    hipLaunchKernelGGL(preview_gather_kernel, dim3(4, n), dim3(256), 0, s, p);
    HIPCHECK(c, hipGetLastError());
    return HD_OK;
}

static std::vector<Op>* which_program(hd_ctx* c, int which) {
    static std::vector<Op> empty;
    if (c->cr) return &c->ws->cr_prog.ops;
    if (c->vae) return which == 0 ? &c->ws->vae_enc_prog.ops : &c->ws->vae_dec_prog.ops;
    if (c->lpips) return &c->ws->lpips_prog.ops;
    if (c->ws->chains.empty()) return &empty;
    return which == 0 ? &c->ws->chains[0].program : &c->ws->chains[0].prep_program;
}
int hd_num_ops(hd_ctx* c, int which) { return c ? (int)which_program(c, which)->size() : 0; }
int hd_num_chains(hd_ctx* c) { return c ? (int)c->ws->chains.size() : 0; }
int hd_debug_limit_ops(hd_ctx* c, int which, int n) {
    if (!c) return HD_ERR_INVALID;
    (which == 0 ? c->op_limit : c->prep_limit) = n;
    return HD_OK;
}
const char* hd_debug_op_name(hd_ctx* c, int which, int i) {
    if (!c) return "";
    auto* p = which_program(c, which);
    return (i >= 0 && i < (int)p->size()) ? (*p)[i].name.c_str() : "";
}
static int op_info_word(const Op& op) {
    if (!op.gemm || op.lk < 0) return 0;
    return ((op.lk + 1) & 0xff) | (((op.ek + 1) & 0xff) << 8) | (((op.mode + 1) & 0xff) << 16) | ((op.gemm->xcd_tile_affine ? 1 : 0) << 24) |
           ((op.gemm->w_nt ? 1 : 0) << 25);
}
int hd_debug_op_info(hd_ctx* c, int which, int i) {
    if (!c) return HD_ERR_INVALID;
    auto* p = which_program(c, which);
    if (i < 0 || i >= (int)p->size()) HD_FAIL(c, HD_ERR_INVALID, "no such op %d", i);
    return op_info_word((*p)[i]);
}

// One launch of the shared GEMM kernels on the caller's operands (include/hifidiff_hip.h).  Everything the packer or a launcher does
// not take is refused here, before add_gemm: a refused case never becomes a launch.
int hd_debug_gemm(hd_ctx* c, const char* weight, int loader, int epilogue, const hd_gemm_desc* d, int flags, hd_gemm_note* note, void* stream) {
    if (!c) return HD_ERR_INVALID;
    if (!weight || !d || !note) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: weight, desc and note must not be NULL");
    *note = hd_gemm_note{};
    if (c->finalized) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: ctx is finalized (the entry takes a context whose weights are still raw)");
    static const int pairs[][2] = {{LK_F32, EK_BIASF32}, {LK_F32, EK_PIXSHUF}, {LK_BF16, EK_RESID}, {LK_BF16S, EK_RESID}, {LK_BF16, EK_BIASBF16},
                                   {LK_BF16, EK_PIXSHUF}, {LK_BF16, EK_BIASF32}, {LK_LN, EK_GATE}, {LK_LN, EK_BIASF32}};
    bool known = false;
    for (const auto& pr : pairs) known = known || (pr[0] == loader && pr[1] == epilogue);
    if (!known) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: loader %d -> epilogue %d is not a pair the GEMM dispatch builds without face geometry", loader, epilogue);
    const LdKind lk = (LdKind)loader;
    const EpKind ek = (EpKind)epilogue;
    const std::string name = weight;
    const RawTensor* w = find_raw(c, name + ".weight");
    if (!w || !w->dev) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: weight %s.weight has not been loaded", weight);
    if (!(w->shape.size() == 2 || (w->shape.size() == 4 && w->shape[2] == 1 && w->shape[3] == 1)))
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: weight %s.weight must be [N][K] or [N][K][1][1]", weight);
    const int64_t N64 = w->shape[0], K64 = w->shape[1];
    if (N64 < 1 || N64 > (1 << 20) || K64 < 8 || K64 > (1 << 16)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: weight %s.weight: N or K out of range", weight);
    const int N = (int)N64, K = (int)K64;
    if (K % 8 != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: K = %d of weight %s is not a multiple of 8", K, weight);
    const RawTensor* b = find_raw(c, name + ".bias");
    if (b && ((int64_t)b->numel != N64 || !b->dev)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: weight %s.bias must have N = %d elements", weight, N);
    const bool ep_f32 = ek == EK_BIASF32 || ek == EK_RESID || ek == EK_PIXSHUF;
    if (!b && (ek == EK_RESID || ek == EK_GATE || ek == EK_BIASBF16)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: weight %s.bias is missing (the epilogue reads it)", weight);
    if (ek == EK_GATE && N % 64 != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: weight N = %d must be a multiple of 64 for the gate epilogue", N);
    // ---- the descriptor
    if (d->M < 1 || d->M > (1 << 24)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: M = %d out of range", d->M);
    if (d->act < 0 || d->act > 2 || (d->act != 0 && ek != EK_BIASF32 && ek != EK_BIASBF16)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: act = %d (0 - 2; BIASF32 and BIASBF16 only)", d->act);
    const int r = d->shuffle_r;
    if (!(r == 1 || (r == 2 && ek == EK_PIXSHUF))) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: shuffle_r = %d (1, or 2 with the PIXSHUF epilogue)", r);
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    auto bad_ptr = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    auto misaligned = [](const void* p) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
#define HD_NEED(field) do { if (bad_ptr(d->field)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: %s is NULL or not 16-byte aligned", #field); } while (0)
#define HD_OPT(field) do { if (misaligned(d->field)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: %s is not 16-byte aligned", #field); } while (0)
#define HD_UNUSED(field) do { if (d->field != nullptr) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: %s is not read or written by this loader / epilogue pair", #field); } while (0)
    HD_NEED(A); HD_NEED(out);
    const int a_elems = lk == LK_F32 ? 4 : 8;                 // elements per 16-byte load of the loader
    if (d->lda < K) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: lda = %d < K = %d", d->lda, K);
    if (d->lda % a_elems != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: lda = %d must be a multiple of %d (16-byte row loads)", d->lda, a_elems);
    const bool faces = lk == LK_BF16S || (lk == LK_LN && d->film_face_stride != 0) || d->outg16 != nullptr;
    if (faces && (d->hw < 1 || d->M % d->hw != 0)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: M = %d is not a multiple of hw = %d (rows are mapped to faces)", d->M, d->hw);
    if (lk == LK_LN) {
        HD_NEED(stats_in); HD_NEED(film);
        if (d->stats_np < 1 || d->stats_cnt < 1 || (int64_t)d->stats_np * d->stats_cnt != K)
            HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: stats_np * stats_cnt = %d * %d != K = %d", d->stats_np, d->stats_cnt, K);
        if (d->film_gain_off < 0 || d->film_bias_off < 0 || d->film_gain_off % 4 != 0 || d->film_bias_off % 4 != 0 || d->film_face_stride < 0 || d->film_face_stride % 4 != 0)
            HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: film_gain_off / film_bias_off / film_face_stride must be non-negative multiples of 4");
        if (d->film_face_stride != 0 && d->face0 < 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: face0 = %d", d->face0);
    } else {
        HD_UNUSED(stats_in); HD_UNUSED(film);
    }
    if (lk == LK_BF16S) HD_NEED(rowscale); else HD_UNUSED(rowscale);
    const int ncols = ek == EK_GATE ? N / 2 : (r == 2 ? N / 4 : N);
    if (r == 2) {
        if (N % 4 != 0 || !pow2(d->Win) || !pow2(d->ldo) || d->ldo != N / 4)
            HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: PixelShuffle r = 2 needs Win = %d and ldo = %d to be powers of two and ldo = N / 4 = %d", d->Win, d->ldo, N / 4);
        if ((int64_t)d->M % ((int64_t)d->Win * d->Win) != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: M = %d is not a multiple of Win^2 = %d (PixelShuffle)", d->M, d->Win * d->Win);
    } else if (d->ldo < ncols) {
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: ldo = %d < %d output columns", d->ldo, ncols);
    }
    if (ek == EK_RESID) {
        HD_NEED(resid); HD_NEED(rscale);
        if (d->ldr < N) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: ldr = %d < N = %d", d->ldr, N);
        if (d->outg16) { HD_NEED(outg16); HD_NEED(gate_c); HD_NEED(gate_s); HD_OPT(add_src); }
        else { HD_UNUSED(gate_c); HD_UNUSED(gate_s); HD_UNUSED(add_src); }
    } else {
        HD_UNUSED(rscale); HD_UNUSED(outg16); HD_UNUSED(gate_c); HD_UNUSED(gate_s); HD_UNUSED(add_src);
        if (ek == EK_BIASBF16) { HD_OPT(resid); if (d->resid && d->ldr < N) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: ldr = %d < N = %d", d->ldr, N); }
        else if (ek == EK_PIXSHUF) HD_OPT(resid);
        else HD_UNUSED(resid);
    }
    if (ep_f32) {
        HD_OPT(out16); HD_OPT(stats_out);
        if (d->stats_out && (N % 32 != 0 || (r == 2 && d->ldo % 32 != 0))) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_gemm: stats_out needs whole 32-column tiles (N = %d, ldo = %d)", N, d->ldo);
    } else {
        HD_UNUSED(out16); HD_UNUSED(stats_out);
    }
#undef HD_NEED
#undef HD_OPT
#undef HD_UNUSED
    // ---- the packed weight (first use: packed on the null stream, then waited for)
    HIPCHECK(c, hipSetDevice(c->device));
    const std::string key = name + (r == 2 ? "#s2" : "");
    auto it = c->dbg_packed.find(key);
    if (it == c->dbg_packed.end()) {
        PackedW pw;
        PackOpts o;
        if (r == 2) o.S2 = 4;
        if (const int rc = pack_weight(c, name, &pw, o)) return rc;
        HIPCHECK(c, hipDeviceSynchronize());
        it = c->dbg_packed.emplace(key, pw).first;
    }
    GemmP p = base_gemm(it->second, d->M);
    p.A = d->A; p.lda = d->lda; p.a_scale = lk == LK_F32 ? d->a_scale : 1.f;
    p.hw = faces ? d->hw : 1; p.face0 = d->face0;
    p.stats_in = reinterpret_cast<const float2*>(d->stats_in);
    if (lk == LK_LN) { p.stats_np = d->stats_np; p.stats_cnt = d->stats_cnt; }
    p.film = d->film; p.film_face_stride = d->film_face_stride; p.film_gain_off = d->film_gain_off; p.film_bias_off = d->film_bias_off;
    p.rowscale = d->rowscale;
    p.out = d->out; p.ldo = d->ldo; p.out16 = static_cast<unsigned short*>(d->out16); p.outg16 = static_cast<unsigned short*>(d->outg16);
    p.stats_out = reinterpret_cast<float2*>(d->stats_out);
    p.resid = d->resid; p.ldr = d->ldr; p.rscale = d->rscale; p.gate_c = d->gate_c; p.gate_s = d->gate_s; p.add_src = d->add_src;
    p.act = d->act; p.shuffle_r = r;
    if (ek == EK_PIXSHUF) { p.bias = nullptr; p.Hin = d->Win; p.Win = d->Win; }
    std::vector<Op> prog;
    add_gemm(c, prog, "debug_gemm." + name, p, lk, ek);
    note->op_info = op_info_word(prog[0]);
    if (flags & HD_GEMM_DRY_RUN) return HD_OK;
    g_launch_note = LaunchNote{};
    if (const int rc = run_ops(c, prog, static_cast<hipStream_t>(stream))) return rc;
    const LaunchNote& ln = g_launch_note;
    note->family = ln.family; note->rows = ln.rows; note->pair = ln.pair; note->wk = ln.wk; note->cpw = ln.cpw; note->nt = ln.nt;
    note->wide_form = ln.wide_form; note->threads = ln.threads; note->grid_x = ln.grid_x; note->grid_y = ln.grid_y;
    return HD_OK;
}
// One launch of a face-geometry convolution on the caller's operands (include/hifidiff_hip.h), through add_hca / add_down: the library
// picks the kernel from (C, side, M) and the note says what ran.  Everything the packer or a launcher does not take is refused first.
// HD_CONV_DWGATE: conv1 -> depthwise 3x3 -> SimpleGate -> pool through add_conv1_dwgate, the function add_naf_block calls
static int debug_dwgate(hd_ctx* c, const char* weight, const char* weight2, const hd_conv_desc* d, int flags, hd_conv_note* note, void* stream) {
    if (!weight2) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight2 (conv2) must not be NULL for HD_CONV_DWGATE");
    const int C = d->C, side = d->side;
    if (side < 1 || side > 64 || (side & (side - 1)) != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: side = %d must be a power of two in [1, 64]", side);
    if (C < 32 || C > 2048 || C % 32 != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: C = %d must be a multiple of 32 in [32, 2048]", C);
    const int HW = side * side;
    if (d->M < 1 || d->M > (1 << 16) || d->M % HW != 0)
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: M = %d must be a multiple of side * side = %d in [1, 65536] (rows are pixels of whole faces)", d->M, HW);
    const int faces = d->M / HW;
    if (d->stats_np < 1 || d->stats_cnt < 1 || (int64_t)d->stats_np * d->stats_cnt != C)
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: stats_np * stats_cnt = %d * %d != C = %d", d->stats_np, d->stats_cnt, C);
    if (d->film_off < 0 || d->film_off % 4 != 0 || d->film_face_stride < 0 || d->film_face_stride % 4 != 0)
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: film_off = %d / film_face_stride = %d must be non-negative multiples of 4", d->film_off, d->film_face_stride);
    if (d->face0 < 0 || d->face0 > (1 << 16)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: face0 = %d", d->face0);
    auto bad_ptr = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
#define HD_NEED(field) do { if (bad_ptr(d->field)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: %s is NULL or not 16-byte aligned", #field); } while (0)
    HD_NEED(X); HD_NEED(stats_in); HD_NEED(film); HD_NEED(G); HD_NEED(pooled); HD_NEED(T1);
#undef HD_NEED
    if (d->pooled16 && (reinterpret_cast<uintptr_t>(d->pooled16) & 15) != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: pooled16 is not 16-byte aligned");
    if (d->out || d->out16 || d->stats_out) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: out, out16 and stats_out are not written by HD_CONV_DWGATE");
    const int64_t t1_need = (int64_t)2 * d->M * C + (int64_t)faces * ((side + 7) / 8) * C;
    if (d->T1_elems < t1_need) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: T1_elems = %lld < %lld", (long long)d->T1_elems, (long long)t1_need);
    // ---- the weights
    const std::string n1 = weight, n2 = weight2;
    const RawTensor *w1 = find_raw(c, n1 + ".weight"), *b1 = find_raw(c, n1 + ".bias"), *w2 = find_raw(c, n2 + ".weight"), *b2 = find_raw(c, n2 + ".bias");
    if (!w1 || !w1->dev || !(w1->shape == Shape{2 * C, C} || w1->shape == Shape{2 * C, C, 1, 1}))
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight %s.weight must be [%d][%d] or [%d][%d][1][1] for C = %d", weight, 2 * C, C, 2 * C, C, C);
    if (!b1 || !b1->dev || (int64_t)b1->numel != 2 * C) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight %s.bias must have %d elements", weight, 2 * C);
    if (!w2 || !w2->dev || w2->shape != Shape{2 * C, 1, 3, 3})
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight2 %s.weight must be [%d][1][3][3] for C = %d", weight2, 2 * C, C);
    if (!b2 || !b2->dev || (int64_t)b2->numel != 2 * C) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight2 %s.bias must have %d elements", weight2, 2 * C);
    HIPCHECK(c, hipSetDevice(c->device));
    BlockW bw;
    bw.name = "debug_conv." + n1; bw.C = C; bw.film_off = d->film_off;
    auto it = c->dbg_packed.find(n1 + "#conv");
    if (it == c->dbg_packed.end()) {
        PackedW pw;
        if (const int rc = pack_weight(c, n1, &pw)) return rc;
        HIPCHECK(c, hipDeviceSynchronize());
        it = c->dbg_packed.emplace(n1 + "#conv", pw).first;
    }
    bw.conv1 = it->second;
    bw.dw_w = w2->dev; bw.dw_b = b2->dev;
    it = c->dbg_packed.find(n2 + "#dwT");                       // the tap-major copy, kept in the bias slot of a PackedW without a weight
    if (it == c->dbg_packed.end()) {
        if (const int rc = make_dw_layout(c, bw)) return rc;
        HIPCHECK(c, hipDeviceSynchronize());
        PackedW pw;
        pw.bias = bw.dw_wT;
        it = c->dbg_packed.emplace(n2 + "#dwT", pw).first;
    }
    bw.dw_wT = it->second.bias;
    Level lv{};
    lv.C = C; lv.H = side; lv.M = d->M;
    lv.Xb = const_cast<unsigned short*>(static_cast<const unsigned short*>(d->X));
    lv.sx = reinterpret_cast<float2*>(const_cast<float*>(d->stats_in));
    lv.G = static_cast<unsigned short*>(d->G); lv.pooled = d->pooled; lv.pooled16 = static_cast<unsigned short*>(d->pooled16); lv.T1 = d->T1;
    std::vector<Op> prog;
    const bool strips = add_conv1_dwgate(c, prog, bw, lv, d->film, d->face0, d->stats_np, d->stats_cnt, d->film_face_stride);
    note->dw_path = strips ? 2 : (prog.size() == 3 ? 3 : 1);
    note->hint = -1;
    note->gemm.op_info = op_info_word(prog[0]);
    if (flags & HD_GEMM_DRY_RUN) return HD_OK;
    g_launch_note = LaunchNote{};
    if (const int rc = run_ops(c, prog, static_cast<hipStream_t>(stream))) return rc;
    if (!strips) {
        const LaunchNote& ln = g_launch_note;
        hd_gemm_note& g = note->gemm;
        g.family = ln.family; g.rows = ln.rows; g.pair = ln.pair; g.wk = ln.wk; g.cpw = ln.cpw; g.nt = ln.nt;
        g.wide_form = ln.wide_form; g.threads = ln.threads; g.grid_x = ln.grid_x; g.grid_y = ln.grid_y;
        note->threads = ln.threads; note->grid_x = ln.grid_x; note->grid_y = ln.grid_y;
    }
    note->form = 3;
    return HD_OK;
}

int hd_debug_conv(hd_ctx* c, int kind, const char* weight, const char* weight2, const hd_conv_desc* d, int flags, hd_conv_note* note, void* stream) {
    if (!c) return HD_ERR_INVALID;
    if (!weight || !d || !note) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight, desc and note must not be NULL");
    *note = hd_conv_note{};
    if (c->finalized) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: ctx is finalized (the entry takes a context whose weights are still raw)");
    if (kind == HD_CONV_DWGATE) return debug_dwgate(c, weight, weight2, d, flags, note, stream);
    if (kind != HD_CONV_HCA && kind != HD_CONV_DOWN) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: kind = %d (HD_CONV_HCA, HD_CONV_DOWN or HD_CONV_DWGATE)", kind);
    if (weight2) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight2 is not read by kind %d", kind);
    const bool down = kind == HD_CONV_DOWN;
    // ---- the geometry
    const int C = d->C, side = d->side;
    // (the range of the programs' levels and of the tests: with M <= 2^16 and C <= 2^11 no 32-bit index of a loader or an epilogue wraps)
    if (side < (down ? 2 : 1) || side > 32 || (side & (side - 1)) != 0)
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: side = %d must be a power of two in [%d, 32]", side, down ? 2 : 1);
    if (C < 32 || C > 2048 || C % 32 != 0) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: C = %d must be a multiple of 32 in [32, 2048]", C);
    const int HW = side * side;
    if (d->M < 1 || d->M > (1 << 16) || d->M % HW != 0)
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: M = %d must be a multiple of side * side = %d in [1, 65536] (rows are pixels of whole faces)", d->M, HW);
    auto bad_ptr = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    auto misaligned = [](const void* p) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (bad_ptr(d->X)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: X is NULL or not 16-byte aligned");
    if (bad_ptr(d->out)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: out is NULL or not 16-byte aligned");
    if (misaligned(d->out16)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: out16 is not 16-byte aligned");
    if (misaligned(d->stats_out)) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: stats_out is not 16-byte aligned");
    if (!down && d->stats_out) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: stats_out is not written by HD_CONV_HCA");
    // ---- the weight
    const std::string name = weight;
    const RawTensor* w = find_raw(c, name + ".weight");
    if (!w || !w->dev) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight %s.weight has not been loaded", weight);
    const int N = down ? 2 * C : C, kk = down ? 2 : 3;
    if (w->shape != Shape{N, C, kk, kk})
        HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight %s.weight must be [%d][%d][%d][%d] for C = %d", weight, N, C, kk, kk, C);
    const RawTensor* b = find_raw(c, name + ".bias");
    if (!b || !b->dev || (int64_t)b->numel != N) HD_FAIL(c, HD_ERR_INVALID, "hd_debug_conv: weight %s.bias must have %d elements", weight, N);
    // ---- the packed weight (first use: packed on the null stream, then waited for)
    HIPCHECK(c, hipSetDevice(c->device));
    const bool centre = !down && side == 1;                   // 1x1 map: only the centre tap sees data (as finalize packs hcas of such a level)
    const std::string key = name + (centre ? "#centre" : "#conv");
    auto it = c->dbg_packed.find(key);
    if (it == c->dbg_packed.end()) {
        PackedW pw;
        PackOpts o;
        o.centre_only = centre;
        if (const int rc = pack_weight(c, name, &pw, o)) return rc;
        HIPCHECK(c, hipDeviceSynchronize());
        it = c->dbg_packed.emplace(key, pw).first;
    }
    std::vector<Op> prog;
    if (down) {
        Level src{}, dst{};
        src.C = C; src.H = side; src.M = d->M; src.Xb = const_cast<unsigned short*>(static_cast<const unsigned short*>(d->X));
        dst.C = N; dst.H = side / 2; dst.M = d->M / 4; dst.X = d->out; dst.Xb = static_cast<unsigned short*>(d->out16);
        dst.sx = reinterpret_cast<float2*>(d->stats_out);
        add_down(c, prog, "debug_conv." + name, it->second, src, dst);
    } else {
        HcaW hw;
        hw.C = C; hw.fused = it->second; hw.centre_only = centre;
        add_hca(c, prog, "debug_conv." + name, hw, static_cast<const unsigned short*>(d->X), d->out, static_cast<unsigned short*>(d->out16), d->M, side);
    }
    note->centre_only = centre ? 1 : 0;
    note->hint = prog[0].hint;
    note->gemm.op_info = op_info_word(prog[0]);
    if (flags & HD_GEMM_DRY_RUN) return HD_OK;
    g_launch_note = LaunchNote{};
    g_conv_note = ConvLaunchNote{};
    if (const int rc = run_ops(c, prog, static_cast<hipStream_t>(stream))) return rc;
    if (prog[0].gemm) {
        const LaunchNote& ln = g_launch_note;
        hd_gemm_note& g = note->gemm;
        note->form = 2;
        g.family = ln.family; g.rows = ln.rows; g.pair = ln.pair; g.wk = ln.wk; g.cpw = ln.cpw; g.nt = ln.nt;
        g.wide_form = ln.wide_form; g.threads = ln.threads; g.grid_x = ln.grid_x; g.grid_y = ln.grid_y;
        note->threads = ln.threads; note->grid_x = ln.grid_x; note->grid_y = ln.grid_y;
    } else {
        const ConvLaunchNote& cn = g_conv_note;
        note->form = 1;
        note->C = cn.C; note->side = cn.S; note->bm = cn.BM; note->mt = cn.MT; note->ks = cn.KS; note->nt = cn.NT; note->strip = cn.strip;
        note->depth = cn.depth; note->faces_per_wg = (!cn.strip && cn.BM > cn.S * cn.S) ? cn.BM / (cn.S * cn.S) : 1;
        note->threads = cn.threads; note->grid_x = cn.grid_x; note->grid_y = cn.grid_y; note->remap = cn.remap;
    }
    return HD_OK;
}
static int64_t read_to_host(hd_ctx* c, const void* dev, size_t n, int is_bf16, float* host_out, int64_t max_elems) {
    if (!host_out) return (int64_t)n;
    if ((int64_t)n > max_elems) HD_FAIL(c, HD_ERR_INVALID, "debug read needs %zu elements", n);
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipDeviceSynchronize());
    if (is_bf16) {
        std::vector<unsigned short> tmp(n);
        HIPCHECK(c, hipMemcpy(tmp.data(), dev, n * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) { unsigned u = (unsigned)tmp[i] << 16; memcpy(&host_out[i], &u, 4); }
    } else {
        HIPCHECK(c, hipMemcpy(host_out, dev, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return (int64_t)n;
}
int64_t hd_debug_read_op(hd_ctx* c, int which, int i, float* host_out, int64_t max_elems) {
    if (!c) return HD_ERR_INVALID;
    auto* p = which_program(c, which);
    if (i < 0 || i >= (int)p->size() || !(*p)[i].out) HD_FAIL(c, HD_ERR_INVALID, "no such op %d", i);
    return read_to_host(c, (*p)[i].out, (*p)[i].out_elems, (*p)[i].out_bf16, host_out, max_elems);
}

// a named buffer of the active workspace, else one of the context's own
static const std::pair<void*, std::pair<size_t, int>>* find_debug(hd_ctx* c, const char* name) {
    for (const auto* m : {&c->ws->dbg, &c->dbg}) {
        const auto it = m->find(name);
        if (it != m->end()) return &it->second;
    }
    return nullptr;
}

int64_t hd_debug_read(hd_ctx* c, const char* name, float* host_out, int64_t max_elems) {
    if (!c || !name) return HD_ERR_INVALID;
    // the per-face extras belong to the context, not to a workspace: sized by the batch in use (guide_scale, preview_rows: the int32
    // values as they are, 4 bytes each)
    const size_t B = (size_t)c->ws->B, ll = (size_t)c->L * c->L;
    const bool mk = c->mask.dmask && c->ws->B >= 1 && c->ws->B <= c->mask.cap, gd = c->guide.lp && c->ws->B >= 1 && c->ws->B <= c->guide.cap;
    const bool pv = c->preview.active(c);
    const char *no_mask = "no mask has been set for this batch", *no_guide = "no guidance has been set for this batch";
    const char* no_pv = "previews are off or no batch has been prepared since";
    const struct { const char* name; const void* ptr; size_t elems; bool ok; const char* why; } extras[] = {
        {"mask", c->mask.dmask, B * ll, mk, no_mask}, {"mask_known", c->mask.dknown, B * 4 * ll, mk, no_mask},
        {"mask_noise", c->mask.dnoise, B * 4 * ll, mk, no_mask},
        {"guide_lp", c->guide.lp, B * 4 * ll, gd, no_guide}, {"guide_weight", c->guide.w, B, gd, no_guide}, {"guide_scale", c->guide.n, B, gd, no_guide},
        {"x0_preview", c->preview.x0, B * 4 * ll, pv, no_pv}, {"preview_rows", c->preview.row, B, pv, no_pv},
        {"preview_snaps", c->preview.snap, (size_t)c->preview.snaps * B * 4 * ll, pv, no_pv},
    };
    for (const auto& x : extras) {
        if (strcmp(name, x.name) != 0) continue;
        if (!x.ok) HD_FAIL(c, HD_ERR_INVALID, "debug buffer %s: %s", name, x.why);
        return x.elems ? read_to_host(c, x.ptr, x.elems, 0, host_out, max_elems) : 0;      // preview_snaps without snapshot planes
    }
    const auto* e = find_debug(c, name);
    if (!e) HD_FAIL(c, HD_ERR_INVALID, "unknown debug buffer %s", name);
    return read_to_host(c, e->first, e->second.first, e->second.second, host_out, max_elems);
}

int hd_debug_write(hd_ctx* c, const char* name, const float* host_in, int64_t n_elems) {
    if (!c || !name || !host_in) return HD_ERR_INVALID;
    const auto* e = find_debug(c, name);
    if (!e) HD_FAIL(c, HD_ERR_INVALID, "unknown debug buffer %s", name);
    const size_t n = e->second.first;
    if ((int64_t)n != n_elems) HD_FAIL(c, HD_ERR_INVALID, "debug write of %s needs %zu elements", name, n);
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipDeviceSynchronize());
    if (e->second.second) {                        // bf16 buffer: round to nearest even, as the kernels do
        std::vector<unsigned short> tmp(n);
        for (size_t i = 0; i < n; ++i) {
            unsigned u; memcpy(&u, &host_in[i], 4);
            if ((u & 0x7fffffffu) > 0x7f800000u) { tmp[i] = (unsigned short)((u >> 16) | 0x40u); continue; }   // NaN stays NaN
            tmp[i] = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
        HIPCHECK(c, hipMemcpy(e->first, tmp.data(), n * 2, hipMemcpyHostToDevice));
    } else {
        HIPCHECK(c, hipMemcpy(e->first, host_in, n * sizeof(float), hipMemcpyHostToDevice));
    }
    return HD_OK;
}

int hd_set_option(hd_ctx* c, const char* key, int value) {
    if (!c || !key) return HD_ERR_INVALID;
    const std::string k = key;
    if (k == "xcd") c->xcd_on = value != 0;
    else if (k == "xcd2") c->xcd2_on = value != 0;
    else if (k == "xcd_phase_limit") c->xcd_phase_limit = value;
    else if (k == "xcd_force_global") c->xcd_force_global = value;
    else if (k == "face") c->face_on = value != 0;
    else if (k == "face_block_limit") c->face_block_limit = value;
    else if (k == "stage_limit_first") c->stage_limit_first = value;
    else if (k == "stage_test_abort") c->stage_test_abort = value;   // fault injection: 1..: XCD stages, group 0 gives up its wait for phase value - 1; 1000 + b: face stages, face 0, block b; 2000 + p: a loader wave of hd_xcd2.hpp, phase p
    else HD_FAIL(c, HD_ERR_INVALID, "unknown option %s", key);
    invalidate_step_graphs(c);                             // captured graphs hold the old choice
    return HD_OK;
}
int hd_get_option(hd_ctx* c, const char* key) {
    if (!c || !key) return HD_ERR_INVALID;
    const std::string k = key;
    if (k == "xcd") return (c->xcd_ok && c->xcd_on) ? 1 : 0;
    if (k == "xcd2") return (c->xcd_ok && c->xcd_on && c->xcd2_on) ? c->xcd2_mask : 0;
    if (k == "xcd_stages") return (int)c->xstages.size();
    if (k == "face_stages") return (int)c->fstages.size();
    if (k == "face_l1_rows") return c->face_l1_rows;
    // persistent-stage launches (face-cluster and XCD-local) recorded by the last one-step capture of hd_sample* / hd_sample_rows* (-1: none
    // yet): a stage op that falls back to its per-block launches is not counted
    if (k == "sample_stage_launches") return c->sample_stages;
    if (k == "sample_face_stage_launches") return c->sample_face_stages;
    if (k == "rows_stage_launches") return c->rows_stages;
    if (k == "masked_faces") return c->mask.faces.valid_for(c->ws->B) ? c->mask.faces.count() : 0;   // faces that carry a mask (hd_mask_faces)
    if (k == "preview") return c->preview.on ? 1 : 0;                 // hd_preview_config
    if (k == "guide") return c->guide.on ? 1 : 0;                // hd_guide_config
    if (k == "guided_faces") return c->guide.faces.valid_for(c->ws->B) ? c->guide.faces.count() : 0;   // faces that are guided (hd_guide_faces)
    if (k == "pool_capacity") return c->pool_cap;                // hd_pool_config
    if (k == "pool_valid") { int n = 0; for (char v : c->pool_ok) n += v != 0; return n; }   // entries that hold a prepared face
    if (k == "graph_captures") return c->graph_captures;         // step graphs instantiated by this context (hd_prepare_slots adds none)
    // the folds of the program built for the batch in use (0 before the first call): the decisions build_denoiser_program made, and
    // whether the launch that carries them still runs -- the face-stage entries need the face stages on and a single chain
    const Chain* ch = c->ws->chains.empty() ? nullptr : &c->ws->chains[0];
    const bool face_runs = c->xcd_ok && c->face_on && c->ws->chains.size() == 1;
    if (k == "intro_fold") return (ch && ch->fold_intro && face_runs) ? 1 : 0;
    if (k == "down_fold") return (ch && ch->fold_down0 && face_runs) ? 1 : 0;
    if (k == "up_fold") return (ch && ch->fold_up && face_runs) ? 1 : 0;
    if (k == "end_fold") return (ch && ch->fuse_end && c->end_fused) ? 1 : 0;
    return HD_ERR_INVALID;
}

// To be called after the caller has synchronised the stream its hd_eps / hd_sample calls ran on: reports (once) a persistent
// stage that gave up during one of them.  The reference raises RuntimeError synchronously (test_refiner.py:89-91);
// here the call is asynchronous, its result is NaN-poisoned on the device, and this is where the error surfaces on the host.
int hd_check(hd_ctx* c) {
    if (!c) return HD_ERR_INVALID;
    return check_xcd(c);
}

int hd_set_profiling(hd_ctx* c, int on) { if (!c) return HD_ERR_INVALID; c->profiling = on != 0; return HD_OK; }

int hd_get_profile(hd_ctx* c, double* loop_ms, double* step_ms_avg, int64_t* weight_bytes_per_step, double* flops_per_face_step) {
    if (!c) return HD_ERR_INVALID;
    float ms = 0.f;
    if (c->profiling && c->last_steps > 0) {
        HIPCHECK(c, hipEventSynchronize(c->ev1));
        HIPCHECK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    }
    if (loop_ms) *loop_ms = ms;
    if (step_ms_avg) *step_ms_avg = c->last_steps > 0 ? ms / c->last_steps : 0.0;
    if (weight_bytes_per_step) *weight_bytes_per_step = c->weight_bytes_per_step;
    if (flops_per_face_step) *flops_per_face_step = c->flops_per_face_step;
    return HD_OK;
}

}  // extern "C"
