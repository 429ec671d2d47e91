/*
 * hifidiff_hip.h — C-ABI of the MI355X-native HifiDiff refiner sampling path.
 *
 * The reference (js43o/HifiDiff) has no FFI/plugin interface: its boundary for this path is the
 * Python nn.Module surface called from the sampling loop.  Each entry point below names the
 * reference interface it replaces (file:line into the reference tree).  Plain pointers and sizes
 * only; no torch types.  All tensors are fp32, NCHW-contiguous, DEVICE pointers unless stated.
 * Every call enqueues its work on `stream` (a hipStream_t, passed as void*) and returns without
 * synchronising, except where noted.  Return value: 0 on success, negative hd_status on error;
 * the message is available from hd_last_error().  A context is not thread-safe; use one per device.
 */
#ifndef HIFIDIFF_HIP_H
#define HIFIDIFF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hd_ctx hd_ctx;

enum hd_status {
    HD_OK = 0,
    HD_ERR_INVALID = -1,   /* bad argument / shape / state              */
    HD_ERR_HIP = -2,       /* a HIP runtime call failed                  */
    HD_ERR_WEIGHTS = -3,   /* missing / unexpected / mis-shaped tensor   */
    HD_ERR_NOT_READY = -4  /* weights not loaded or batch not prepared   */
};

/* One state-dict entry.  Replaces `model.load_state_dict(load_file(ckpt))`
 * (test_refiner.py:162-164, models/refiner.py:18-25): same key names and shapes as
 * FacialRefiner(latent_res).state_dict(). */
typedef struct hd_tensor_desc {
    const char* name;       /* e.g. "denoiser.middle_blks.3.conv1.weight" */
    const void* data;       /* fp32 (int64 for *.num_batches_tracked, ignored) */
    int32_t ndim;
    int64_t shape[4];
    int32_t is_device;      /* 0: host pointer, 1: device pointer on the context's device */
} hd_tensor_desc;

/* Reverse-diffusion schedule in coefficient form (one row per step, host memory).
 * Replaces `scheduler.set_timesteps(n)` + `scheduler.step(eps, t, x)` of diffusers 0.32.2 as used at
 * test_refiner.py:85-91 (DDIM, eta 0) and the DDPM step of BASELINE's 1000-step configuration:
 *     x0     = clamp((x - c[0]*eps) / c[1], -c[2], +c[2])
 *     x_prev = c[3]*x0 + c[4]*x + c[5]*eps + c[6]*z          z ~ N(0, I)
 */
typedef struct hd_schedule {
    int32_t n_steps;
    const float* timesteps;   /* [n_steps] value fed to the time embedding at each step          */
    const float* coef;        /* [n_steps][7]                                                     */
} hd_schedule;

/* Multistep schedule: the coefficient form above plus one history term, h = the previous step's x0 of the same element.
 * Replaces diffusers' DPMSolverMultistepScheduler (DPM-Solver++ 2M / SDE-DPM-Solver++ 2M, Lu et al. 2022, arXiv 2211.01095)
 * swapped in for DDIMScheduler in the same loop:
 *     x0     = clamp((x - c[0]*eps) / c[1], -c[2], +c[2])
 *     x_prev = c[3]*x0 + c[4]*x + c[5]*eps + c[6]*z + c[7]*h          then  h <- x0
 * h is read only where c[7] != 0; row 0 must have c[7] == 0 (the history of a call starts at its first step). */
typedef struct hd_schedule_ms {
    int32_t n_steps;
    const float* timesteps;   /* [n_steps]                                                        */
    const float* coef;        /* [n_steps][8]                                                     */
} hd_schedule_ms;

/* FacialRefiner(latent_res) (models/refiner.py:11-16): builds the network description for latent
 * side `latent_res` (16 for 16->128 px, 32 for 32->256 px, 64 for 64->512 px) on HIP device `device`.
 * Any other value returns HD_ERR_INVALID before the first HIP call (hd_last_error(NULL) names the accepted
 * sizes): every level side latent_res >> l, l = 0..4, must be a power of two. */
int hd_create(hd_ctx** out, int latent_res, int device);
/* The unconditional pre-training network `Denoiser(latent_size)` (models/denoiser/model.py:32-134; sampled by
 * pretrain_denoiser.py:76-120): the same UNet without priors, HCAs and identity term.  Its state-dict keys are
 * passed with the prefix "denoiser." (denoiser.time_mlp.1.weight, denoiser.encoders.0.0.conv1.weight ...).
 * Use hd_prepare_unconditional instead of hd_prepare; hd_eps / hd_sample work as for the refiner. */
int hd_create_unconditional(hd_ctx** out, int latent_res, int device);
/* The coarse-restoration network that produces `cr_face` before the loop:
 * `CoarseRestoration()` (models/cr/model.py:33-88; called as `cr_module(ln_face)` at test_refiner.py:77,
 * infer_cr.py:48-60).  A context of its own: load its state dict (keys as in the reference, no prefix) with
 * hd_load_weights / hd_finalize_weights, then
 *   hd_cr_forward(ctx, B, ln_face [B,3,128,128], cr_face_out [B,3,128,128], stream). */
int hd_cr_create(hd_ctx** out, int device);
int hd_cr_forward(hd_ctx* ctx, int batch, const float* ln_face, float* cr_face_out, void* stream);

/* VAE boundary either side of the loop: replaces
 *   cr_latent = vae.encode(F.interpolate(cr_face, image_res, mode="bicubic")).latent_dist.sample() * 0.18215
 *                                                              (test_refiner.py:78-83; train_refiner.py:72-83 with to_vae_range)
 *   images    = vae.decode(latent / 0.18215).sample            (test_refiner.py:93; train_refiner.py:122-123)
 * with diffusers' AutoencoderKL of "stable-diffusion-2-1-base" (third party; weights come from the caller's state dict with
 * diffusers' key names, loaded with hd_load_weights / hd_finalize_weights on a context from hd_vae_create).
 *   hd_vae_encode: images [B,3,in_res,in_res] fp32 NCHW; bicubic (align_corners=False) to image_res when they differ;
 *                  vae_range 1 applies clamp(0,1)*2-1 first; moments_out [B,8,L,L] (mean | logvar of the posterior) and / or
 *                  latents_out [B,4,L,L] = (mean + std * z) * 0.18215 with z = noise [B,4,L,L] or device Philox(seed); L = image_res/8.
 *   hd_vae_decode: latents [B,4,L,L] -> images_out [B,3,8L,8L]. */
int hd_vae_create(hd_ctx** out, int device);
int hd_vae_encode(hd_ctx* ctx, int batch, int in_res, int image_res, const float* images, int vae_range, const float* noise, uint64_t seed,
                  float* moments_out, float* latents_out, void* stream);
int hd_vae_decode(hd_ctx* ctx, int batch, int latent_res, const float* latents, float* images_out, void* stream);
void hd_destroy(hd_ctx* ctx);
const char* hd_last_error(const hd_ctx* ctx);   /* ctx may be NULL: creation errors */

/* load_state_dict (strict): may be called several times with partial lists; hd_finalize_weights
 * checks that every key of FacialRefiner.state_dict() arrived with the right shape, folds eval-mode
 * BatchNorm into the adjacent conv, and packs all GEMM weights to bf16 MFMA-fragment order.
 * Synchronous (weight ingest is not on the hot path). */
int hd_load_weights(hd_ctx* ctx, const hd_tensor_desc* tensors, int n);
int hd_finalize_weights(hd_ctx* ctx);

/* Once-per-batch conditioning, hoisted out of the loop: `self.fpg(cr_latent)`, `self.idc(cr_face)`
 * (models/refiner.py:33-34), the HCA gates w_c / w_s (models/fpg/hca.py:26-27,33-48) and
 * `idc_conv(identity_embedding)` (models/denoiser/model.py:245).
 *   cr_latent [B,4,L,L]; cr_face [B,3,128,128] or NULL; id_emb [B,2048] or NULL (exactly one of
 *   cr_face / id_emb must be given: id_emb is what FusedDenoiser.forward receives directly). */
int hd_prepare(hd_ctx* ctx, int batch, const float* cr_latent, const float* cr_face,
               const float* id_emb, void* stream);
/* Unconditional Denoiser: `model(latents, t)` has nothing to hoist; this sizes the workspace for `batch`
 * latents and builds the launch program (pretrain_denoiser.py:101-110). */
int hd_prepare_unconditional(hd_ctx* ctx, int batch, void* stream);

/* Same, but from already-computed priors: FusedDenoiser.forward(latents, timesteps, facial_priors,
 * identity_embedding) (models/denoiser/model.py:217).  priors[i] is NCHW
 * [B, 2048>>i, (L/16)<<i, (L/16)<<i]. */
int hd_prepare_from_priors(hd_ctx* ctx, int batch, const float* const priors[5],
                           const float* id_emb, void* stream);

/* The two conditioning extractors on their own, for callers that use `model.fpg(cr_latent)` /
 * `model.idc(cr_face)` directly (models/refiner.py:33-34; FacialPriorGuidance.forward
 * models/fpg/model.py:46-64, ResNet.forward models/idc/model.py:122-135).
 *   priors_out[i]: NCHW [B, 2048>>i, (L/16)<<i, (L/16)<<i];  id_emb_out: [B,2048] (== (B,2048,1,1)). */
int hd_fpg(hd_ctx* ctx, int batch, const float* cr_latent, float* const priors_out[5], void* stream);
int hd_idc(hd_ctx* ctx, int batch, const float* cr_face, float* id_emb_out, void* stream);

/* One denoiser evaluation: FusedDenoiser.forward (models/denoiser/model.py:217-266) on the prepared
 * batch.  x, eps_out [B,4,L,L]; timesteps: n_t == 1 (shared) or n_t == B values, device fp32. */
int hd_eps(hd_ctx* ctx, const float* x, const float* timesteps, int n_t, float* eps_out, void* stream);

/* The whole reverse-diffusion loop (test_refiner.py:87-91 / train_refiner.py:111-120) on the
 * prepared batch, in latent space, x updated in place.  The per-step kernel sequence is captured
 * once into a hipGraph and replayed n_steps times.
 *   noise: [n_steps][B,4,L,L] device fp32 (z for every step; rows whose c[6]==0 are not read), or
 *          NULL to draw z on the device from Philox4x32-10(seed; step, element). */
int hd_sample(hd_ctx* ctx, float* x_inout, const hd_schedule* sched, const float* noise,
              uint64_t seed, void* stream);
/* The same loop with a multistep schedule (hd_schedule_ms): same graph, noise layout, Philox keying and hd_check semantics
 * as hd_sample.  The x0 history lives in the context's workspace ("x0_hist", [B,4,L,L]) and is per call.
 * HD_ERR_INVALID if row 0 has c[7] != 0. */
int hd_sample_multistep(hd_ctx* ctx, float* x_inout, const hd_schedule_ms* sched, const float* noise,
                        uint64_t seed, void* stream);

/* Per-face schedule positions: the same loop where every face f starts at its own row r_f = start_rows[f] (host [B], 0 <= r_f <= n_steps)
 * of one shared table.  Replaces diffusers' img2img convention -- `get_timesteps(num_inference_steps, strength)` + `scheduler.add_noise(
 * init_latents, noise, timesteps[t_start])`, then the loop of test_refiner.py:85-91 over the remaining rows -- with one strength per face,
 * and a loop split over several calls (preview / cancel / time-slicing).  The call runs n_iters iterations, 1 <= n_iters <= n_steps - min r_f:
 * at iteration i face f is evaluated at row k = r_f + i (timesteps[k], FiLM row k, coefficient row k, z = noise[k] or Philox(seed; k, element),
 * so all r_f = 0 and n_iters = n_steps is hd_sample bit for bit); from k = n_steps on the face is held (its latents are not written).
 * The step graphs of this form are captured on first use, next to hd_sample's.  HD_ERR_INVALID for a row or n_iters out of range. */
int hd_sample_rows(hd_ctx* ctx, float* x_inout, const hd_schedule* sched, const int32_t* start_rows, int n_iters, const float* noise,
                   uint64_t seed, void* stream);
/* The same with a multistep schedule (hd_sample_multistep; a held face's history is not written either).  resume = 0: each face's history
 * starts at its own first row, which is taken first-order as diffusers' img2img does: h := x0 there, so x0 is multiplied by c[3] + c[7].  resume = 1: the history the previous multistep call on this context left for
 * this batch is continued, so a loop split over calls (start rows advanced by the caller) reproduces the one-call loop bit for bit;
 * HD_ERR_INVALID when there is none (no earlier multistep call, hd_prepare* since, another batch size, or hd_sample / hd_sample_rows in between). */
int hd_sample_rows_multistep(hd_ctx* ctx, float* x_inout, const hd_schedule_ms* sched, const int32_t* start_rows, int n_iters, int resume,
                             const float* noise, uint64_t seed, void* stream);

/* Continuous batching (a serving loop that refills the slots of finished faces while the others go on).
 * hd_prepare_slots: replace the conditioning of n faces of the prepared batch: slots[j] (host [n], distinct, in [0, B)) gets the conditioning
 * of cr_latent[j] [4,L,L] and cr_face[j] [3,128,128] (or id_emb[j] [2048]; exactly one of the two), bit for bit what hd_prepare computes for
 * these n faces as a batch of n.  The other slots' conditioning is not touched, captured graphs stay valid (nothing is recaptured), and the
 * prologue runs for the n faces only.  The refilled slots have no multistep history (and hd_sample_rows_multistep(resume = 1) is refused
 * until every face has one again).  HD_ERR_NOT_READY without a prepared conditional batch; HD_ERR_INVALID for a duplicate or out-of-range
 * slot, n outside [1, B], an unconditional / CoarseRestoration / VAE context or a bad pointer combination. */
int hd_prepare_slots(hd_ctx* ctx, int n, const int32_t* slots, const float* cr_latent, const float* cr_face, const float* id_emb, void* stream);
/* The conditioning pool: hd_prepare_slots in two halves, with a place to keep prepared conditioning between them.  The requests waiting in
 * a serving loop's queue are known long before a slot frees, and the prologue costs about the same for 64 faces as for one: prepare
 * them together, and a refill is one copy launch.  Everything stays on the caller's one stream.
 * hd_pool_config: the context owns `capacity` entries (0 <= capacity <= 4096; 0 frees the pool), each one face's conditioning: 5 priors,
 * 5 w_c, 5 w_s, the idc term and id_emb -- about 72 k floats (0.29 MB) at latent 16, 270 k (1.1 MB) at latent 32.  The pool belongs to the
 * context, not to a batch: it survives hd_prepare* (at another batch size too).  (Re)configuring invalidates every entry and may
 * synchronise the device (not for the hot path).  hd_get_option "pool_capacity" / "pool_valid" (entries that hold a face) report it.
 * hd_pool_prepare: run the prologue of hd_prepare_slots for n faces, 1 <= n <= min(B, capacity), and store face j in entry entries[j]
 * (host [n], distinct, in [0, capacity)); cr_latent / cr_face / id_emb as for hd_prepare_slots.  The prologue runs on the prepared batch's
 * staging chain, but nothing of the running batch is written: no slot's conditioning, mask, guidance, preview or history, and nothing is
 * recaptured -- a loop split around the call gives the bits it gives without it.  The entries are valid afterwards; preparing an entry
 * again overwrites it and does not touch a slot it was committed to.
 * hd_pool_commit: copy entry entries[j] (host [n], valid, may repeat: several slots may take one face) into slot slots[j] (host [n],
 * distinct, in [0, B)), 1 <= n <= B, and reset of those slots what hd_prepare_slots resets: mask, guidance, previews, multistep history.
 * Entries stay valid.  Nothing is rebuilt or recaptured.  hd_pool_prepare of n faces followed by commits of them, in any grouping and
 * order, leaves in each slot bit for bit what hd_prepare_slots of the same n faces in the same order leaves: what hd_prepare computes for
 * them as a batch of n.
 * HD_ERR_NOT_READY without a prepared conditional batch or (prepare, commit) without a pool; HD_ERR_INVALID, naming the argument, for an
 * unconditional / CoarseRestoration / VAE context, a capacity or n out of range, a duplicate slot, a duplicate entry in hd_pool_prepare, an
 * out-of-range slot or entry, an entry that was never prepared, or a bad pointer combination. */
int hd_pool_config(hd_ctx* ctx, int capacity);
int hd_pool_prepare(hd_ctx* ctx, int n, const int32_t* entries, const float* cr_latent, const float* cr_face, const float* id_emb, void* stream);
int hd_pool_commit(hd_ctx* ctx, int n, const int32_t* slots, const int32_t* entries, void* stream);
/* hd_sample_rows / hd_sample_rows_multistep with per-face noise keys and per-face resumption (same graphs, hd_check and NaN-poisoning rules).
 * face_seeds: host [B] or NULL.  With it, z of face f at row k, element e of the face (0 <= e < 4L^2) is Philox4x32-10(face_seeds[f]; k, e):
 *   independent of the slot, the batch size and the neighbours -- a face in slot 0 with key s gets exactly the z of hd_sample_rows(seed = s)
 *   for face 0.  NULL: hd_sample_rows' batch keying Philox(seed; k, element of the batch).  noise != NULL overrides both, as before.
 * resume (multistep): host [B] of 0 / 1.  1 continues face f's history; 0 takes its first row first-order (h := x0).  HD_ERR_INVALID if
 *   resume[f] == 1 for a face without a history: none since hd_prepare*, refilled by hd_prepare_slots, or a single-step call since its last
 *   multistep row (hd_sample_multistep leaves every face one, a multistep rows / faces call every face that ran a row; a held face keeps its state). */
int hd_sample_faces(hd_ctx* ctx, float* x_inout, const hd_schedule* sched, const int32_t* start_rows, int n_iters, const uint64_t* face_seeds,
                    const float* noise, uint64_t seed, void* stream);
int hd_sample_faces_multistep(hd_ctx* ctx, float* x_inout, const hd_schedule_ms* sched, const int32_t* start_rows, int n_iters,
                              const int32_t* resume, const uint64_t* face_seeds, const float* noise, uint64_t seed, void* stream);
/* Per-request schedules: mixed step counts and solvers in one batch.  `table` is the concatenation of several schedules in hd_schedule_ms
 * form (a DDIM / DDPM row is the same row with c[7] = 0), and face f owns the span [begin_rows[f], end_rows[f]) of it as its schedule (host
 * [B] each, like start_rows): at iteration i the face is evaluated at row k = start_rows[f] + i while k < end_f and held from then on (its
 * latents, its history and its FiLM row are not written; a masked face's kept region ends exactly on `known` at row end_f - 1).
 *   rows: 0 <= begin_f <= start_f <= end_f <= n_steps; a face with start_f == end_f is held for the whole call (an empty slot).
 *   n_iters in [1, max_f (end_f - start_f)].
 *   every row that is some face's begin must have c[7] == 0 (no history before the first row of a schedule).
 *   resume[f] == 1 continues face f's history under the rules of hd_sample_faces_multistep and needs start_f > begin_f; 0 takes row
 *   start_f first-order.
 *   face_seeds / seed: z of face f at row k is Philox(key; k - begin_f, element): the counter is the row inside the face's own schedule,
 *   so a request's z does not depend on where its schedule sits in the table.  An explicit `noise` tensor [n_steps][B,4,L,L] stays
 *   indexed by the absolute row k of the table.
 * HD_ERR_INVALID, with a message that names the face, for each violation.  With begin_f = 0 and end_f = n_steps for every face this is
 * hd_sample_faces_multistep bit for bit.  The captured per-face graphs are those of hd_sample_rows* / hd_sample_faces* (the spans are read
 * through the loop state: alternating between the entry points captures nothing), and a multistep history is left for every face that ran
 * a row.  The FiLM table of the whole concatenated table is computed once and cached by its timesteps, as for every other entry point; it
 * costs about 0.5 MB per row at latent 16 (0.5 GB for a table of 1000 rows), so a set of long schedules is paid for in memory. */
int hd_sample_spans(hd_ctx* ctx, float* x_inout, const hd_schedule_ms* table, const int32_t* begin_rows, const int32_t* end_rows,
                    const int32_t* start_rows, int n_iters, const int32_t* resume, const uint64_t* face_seeds, const float* noise,
                    uint64_t seed, void* stream);

/* Masked sampling (inpainting, diffusers' inpaint loop for a 4-channel UNet with one mask per face).
 * hd_mask_faces: give n faces of the prepared batch a mask: slots[j] (host [n], distinct, in [0, B); NULL: n == B, faces in order) gets
 * mask[j] [L,L] in [0, 1] (1: resample, 0: keep), known[j] [4,L,L] and known_noise[j] [4,L,L] (device fp32, copied in stream order: the
 * caller's tensors are free once the stream has passed the call).  From then on every hd_sample* call (all six loop entry points) ends the
 * update of row k of such a face with
 *     x <- m * r + (1 - m) * (b0 * known + b1 * known_noise),   r the scheduler update of that element,
 * (b0, b1) = (c[1], c[0]) of row k + 1 -- the signal and noise scale of the row, scheduler.add_noise(known, known_noise, timesteps[k+1]) --
 * and (1, 0) on the last row: the kept region ends exactly on `known`, m == 1 gives r and m == 0 the re-noised known latent bit for bit.
 * The multistep history keeps the unblended x0; a held face is not written.  mask == known == known_noise == NULL clears the masks of the
 * given faces.  Masks stay across hd_sample* calls (a loop split over calls keeps them); every hd_prepare* clears all of them and
 * hd_prepare_slots those of the slots it refills.  Nothing is rebuilt or recaptured, and while no face is masked the step launches read
 * and compute what they did without this call.  hd_eps and hd_scheduler_step* know no mask.  HD_ERR_NOT_READY without a prepared batch;
 * HD_ERR_INVALID for a duplicate or out-of-range slot, n outside [1, B], slots == NULL with n != B, some but not all of the three
 * pointers, or a CoarseRestoration / VAE context. */
int hd_mask_faces(hd_ctx* ctx, int n, const int32_t* slots, const float* mask, const float* known, const float* known_noise, void* stream);

/* Low-pass fidelity guidance (ILVR's low-pass conditioning; the control CodeFormer calls `w` and DiffBIR `g_scale`): how far a face's result
 * may drift from a target -- usually its coarse restoration -- in the low frequencies, while the diffusion adds the detail.
 * hd_guide_config(on): the switch of the context.  While it is on, every step of the loop ends with one small launch more (the guided
 * update, one workgroup per face and channel plane); flipping it makes the captured step graphs stale, so the next hd_sample* call
 * recaptures once.  A context that never switches it on keeps its launches, its graphs and its bits.  on = 0 also stops guiding every face.
 * hd_guide_faces: guide n faces of the prepared batch: slots[j] (host [n], distinct, in [0, B); NULL: n == B, faces in order) is pulled
 * towards target[j] [4,L,L] (device fp32) with weight[j] in (0, 1] and block size scale[j] = N, a divisor of L (host [n] each), on rows
 * row_from[j] <= i < row_to[j] of the face's own schedule (host [n], 0 <= row_from < row_to; both NULL: all rows; i = k - begin_f, the row
 * inside the face's span, begin_f = 0 without hd_sample_spans).  LP_N(target) is computed in stream order by this call and stored: the
 * caller's tensor is free once the stream has passed the call.  On a guided row k of such a face every hd_sample* call (all seven loop
 * entry points) computes, with x, eps, c[0..7], h, z as in hd_schedule / hd_schedule_ms,
 *     x0  = clamp((x - c0*eps)/c1, +-c2)
 *     x0g = x0 + w * (LP_N(target) - LP_N(x0))                 per channel plane
 *     e'  = (x - c1*x0g)/c0                                    where the row uses eps (c5 != 0)
 *     x  <- c3*x0g + c4*x + c5*e' + c6*z + c7*h ;  h <- x0g    (a first-order first row folds c7 into c3, as without guidance)
 * and the mask blend and the preview store follow as they do without guidance (the preview stores x0g).  LP_N of an L x L plane is the
 * mean over each N x N block, upsampled bilinearly back to L x L with align_corners = False: F.interpolate(F.avg_pool2d(x, N), size = L,
 * mode = "bilinear").  N = 1 is the identity (the guidance is element-wise), N = L the plane mean (only each channel's mean is pulled).
 * target == NULL stops guiding the given faces (weight .. row_to are not read).  Setting, changing or clearing faces captures nothing.
 * Lifetime as for the masks: the guidance stays across hd_sample* calls, every hd_prepare* clears all faces and hd_prepare_slots those of
 * the slots it refills.  hd_get_option "guide" returns the switch and "guided_faces" the number of guided faces; hd_debug_read names
 * "guide_lp" [B,4,L,L] (the stored LP_N(target)), "guide_weight" [B] (0: not guided) and "guide_scale" [B] (int32 bits) read the buffers.
 * hd_eps and hd_scheduler_step* know no guidance.  HD_ERR_NOT_READY without a prepared batch; HD_ERR_INVALID for a duplicate or
 * out-of-range slot, n outside [1, B], slots == NULL with n != B, a target while the switch is off, a weight outside (0, 1] or not finite,
 * a scale that does not divide L, row_from >= row_to or row_from < 0, only one of row_from / row_to, or a CoarseRestoration / VAE context. */
int hd_guide_config(hd_ctx* ctx, int on);
int hd_guide_faces(hd_ctx* ctx, int n, const int32_t* slots, const float* target, const float* weight, const int32_t* scale,
                   const int32_t* row_from, const int32_t* row_to, void* stream);

/* Colour correction of decoded faces against a reference image: the step diffusion-based restoration stacks apply after vae.decode
 * (StableSR's wavelet_color_fix / adain_color_fix, shipped unchanged by DiffBIR, SUPIR and SeeSR).  Low-pass guidance acts on the four
 * latent channels during sampling; this call bounds the colour of the decoded RGB image.  The reference project has no such step.
 * images, out [B,3,res,res], ref [B,3,ref_res,ref_res] (device fp32 NCHW); weight: device [B] in [0, 1], or NULL (all 1).  Per face f and
 * channel plane, with c the image plane, s the reference plane and w the face's weight:
 *     s <- clamp(s, 0, 1) * 2 - 1                              with ref_vae_range = 1 (to_vae_range, as hd_vae_encode's vae_range)
 *   mode 1, wavelet with levels = n in 1..5:
 *     s' = F.interpolate(s, res, mode = "bicubic", align_corners = False)    when ref_res != res (the rule hd_vae_encode uses), else s
 *     blur_i(x) = F.conv2d(F.pad(x, (r,r,r,r), mode = "replicate"), k, dilation = r),  r = 2^i,  k = [1/4 1/2 1/4]^T [1/4 1/2 1/4]
 *     B_n = blur_{n-1} o ... o blur_0
 *     out = c + w * B_n(s' - c)
 *   StableSR computes high(c) + low(s) with high(c) = sum_i (c_i - blur_i(c_i)), which telescopes to c - B_n(c); every blur_i is linear,
 *   replicate padding included, so its result is c + B_n(s - c).  Each level runs as a horizontal 3-tap pass then a vertical one, taps
 *   clamped to the image; one launch stages a 64 x 64 tile with its 2^n - 1 halo in LDS and does all 2n passes there.  A pixel's bits do
 *   not depend on the tiling.
 *   mode 2, AdaIN (levels is ignored):
 *     a   = (c - mean(c)) * std(s) / std(c) + mean(s),   std(x) = sqrt(var_unbiased(x) + 1e-5)
 *     out = c + w * (a - c)
 *   with the statistics of s taken at its own resolution (no resampling) and all sums accumulated in fp64.
 * A face with w == 0 gets c bit for bit in either mode.  The call needs no context, allocates nothing, keeps nothing in global memory and
 * does not synchronise: it enqueues one launch on `stream`, and images and ref are only read.  out must not overlap images or ref (a tile
 * reads its neighbours' c).  Errors are reported through hd_last_error(NULL).  HD_ERR_INVALID, naming the argument and before any HIP
 * call, for batch < 1, res or ref_res not a multiple of 64 in [64, 512] (the VAE boundary's range), a mode other than 1 or 2, levels
 * outside [1, 5] in wavelet mode, ref_vae_range outside {0, 1}, a NULL images, out or ref, a pointer that is not aligned to 4 bytes (16
 * bytes for images, out and ref in AdaIN mode), or out overlapping images or ref as byte ranges. */
int hd_color_fix(const float* images, float* out, int batch, int res, const float* ref, int ref_res, int ref_vae_range,
                 int mode, int levels, const float* weight, void* stream);

/* Per-face PSNR and SSIM of images against a reference: what the reference's evaluation loop does with its result (test_refiner.py:113-122:
 * F.interpolate to the target's size, min-max normalise, pyiqa's psnr and ssim).  pyiqa is third party and absent, so parity with its
 * defaults is unpinned, like the schedulers'; the formulas below are the contract.  LPIPS is hd_lpips (below); NIQE needs a fitted model file and is not offered.
 * images [B,3,res,res], ref [B,3,ref_res,ref_res] (device fp32 NCHW; res and ref_res multiples of 64 in [64, 512]).  Everything is scored
 * at the reference's side Rb = ref_res.  Per face:
 *   1. a = F.interpolate(images, Rb, mode = "bicubic", align_corners = False) when res != ref_res (no antialiasing, taps clamped to the
 *      border: the rule hd_vae_encode and hd_color_fix use), else images; b = ref.  The resampling happens while the pixels are loaded.
 *   2. with images_range / ref_range [B,2] (device fp32: lo, hi per face):  x' = (x - lo) / (hi - lo), and x' = 0 where hi <= lo (torch's
 *      (x - min) / (max - min) gives NaN there).  NULL: no normalisation of that tensor.
 *   3. channels = 1 (rgb): the three planes are scored independently, P = 3.
 *      channels = 2 (y):   one plane Y = (65.481 R + 128.553 G + 24.966 B + 16 L) / 255, L = data_range (BT.601 studio luma), P = 1.
 *   4. mse  = mean over the P planes and all Rb^2 pixels of (a' - b')^2.  PSNR = 10 log10(L^2 / mse) is left to the caller (+inf at 0).
 *   5. ssim (Wang et al. 2004) = mean over the P planes and the (Rb - 10)^2 "valid" window positions of
 *        ((2 mu_a mu_b + C1) (2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1) (s_a + s_b + C2)),      C1 = (0.01 L)^2, C2 = (0.03 L)^2,
 *      mu_a, mu_b, E[a^2], E[b^2], E[ab] the window-weighted moments, s_a = E[a^2] - mu_a^2, s_b likewise, s_ab = E[ab] - mu_a mu_b (no
 *      unbiased correction), the window g[k] g[l] with g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1 in float64.
 * out [B,2] (device fp64): mse, ssim.  ssim_map_out: NULL, or device fp32 [B,P,Rb-10,Rb-10] that receives the map of step 5.
 * One launch computes everything per (64 x 64 tile, plane, face): a 74 x 74 region of a' and b' is staged in LDS once, the five moment
 * maps live in registers (fp32 window sums: a horizontal then a vertical 11-tap pass), and the tile's two sums are fp64.  A second, tiny
 * launch adds each face's tile sums in index order.  No atomics: a face's two numbers and its map have the same bits from call to call
 * and at every position of every batch.  workspace: device memory of at least hd_image_metrics_workspace(batch, ref_res, channels) bytes
 * (the tile sums), owned by the caller, overwritten by the call, free to reuse when the call's work on `stream` is done.
 * hd_image_range: range_out [B,2] (device fp32) = the minimum and maximum over the three channels of each face of images as resampled to
 * out_res (step 1; out_res == res: the image itself, and then the result is exactly min / max).  One launch, one workgroup per face.
 * NaN pixels are not propagated (fminf / fmaxf).  Feeding it to images_range / ref_range is `normalize = "face"` of
 * hifidiff_amd.metrics; the batch-wide pair of the reference's loop is the min / max of these over the faces.
 * All three calls need no context, allocate nothing and do not synchronise; the two that launch enqueue on `stream` and only read their
 * inputs.  Errors are reported through hd_last_error(NULL).  HD_ERR_INVALID, naming the argument and before any HIP call, for: batch < 1
 * (hd_image_metrics: > 65535); res, ref_res or out_res not a multiple of 64 in [64, 512]; channels other than 1 or 2; data_range not
 * finite or <= 0; a NULL images, ref, out, range_out or workspace; workspace_bytes too small; a pointer not aligned to 4 bytes (out and
 * workspace: 8 bytes; images of hd_image_range with out_res == res: 16 bytes, it is read as float4); out, ssim_map_out or workspace
 * overlapping an input or each other, range_out overlapping images, as byte ranges.  hd_image_metrics_workspace returns HD_ERR_INVALID
 * for arguments hd_image_metrics would refuse. */
int hd_image_range(const float* images, int batch, int res, int out_res, float* range_out, void* stream);
int64_t hd_image_metrics_workspace(int batch, int ref_res, int channels);
int hd_image_metrics(const float* images, int res, const float* ref, int ref_res, int batch, int channels, float data_range,
                     const float* images_range, const float* ref_range, double* out, float* ssim_map_out, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* Per-face LPIPS (Zhang et al. 2018; AlexNet, v0.1 "lin" weights) of images against a reference: the third score of the reference's
 * evaluation loop (test_refiner.py:107-123, pyiqa.create_metric("lpips")).  The `lpips` package and pyiqa are third party and absent, so
 * parity with them is unpinned, like the schedulers' and the VAE's; the formula below, stated from the paper and from memory of the package,
 * is the contract.  hd_lpips_create makes a context of its own kind, with the life of the others: hd_load_weights, hd_finalize_weights
 * (strict), hd_destroy.  Its manifest, in the package's full-model names:
 *   net.slice1.0 [64,3,11,11], net.slice2.3 [192,64,5,5], net.slice3.6 [384,192,3,3], net.slice4.8 [256,384,3,3], net.slice5.10 [256,256,3,3]
 *   (.weight and .bias [Cout] each);  lin{0..4}.model.1.weight [1,C,1,1], C = 64, 192, 384, 256, 256;  optionally, both or neither,
 *   scaling_layer.shift and scaling_layer.scale [1,3,1,1].
 * images [B,3,res,res], ref [B,3,ref_res,ref_res] (device fp32 NCHW; res and ref_res multiples of 64 in [64, 512]).  Everything is scored
 * at Rb = ref_res.  Per face:
 *   1. a = F.interpolate(images, Rb, mode = "bicubic", align_corners = False) when res != ref_res (step 1 of hd_image_metrics: the same
 *      sampling rule), else images; b = ref.
 *   2. with images_range / ref_range [B,2] (device fp32: lo, hi per face; hd_image_range makes them): x <- (x - lo) / (hi - lo), 0 where
 *      hi <= lo: step 2 of hd_image_metrics.  NULL: no normalisation of that tensor.
 *   3. unit_range = 1: x <- 2x - 1 (the package's normalize=True, pyiqa's default: inputs in [0, 1]).  0: the input is taken as in [-1, 1].
 *   4. the scaling layer: x <- (x - shift_c) / scale_c, shift = (-.030, -.088, -.188), scale = (.458, .448, .450) unless the state dict
 *      carries its own.
 *   5. features, with tap sides s1 = (Rb - 7) / 4 + 1, s2 = (s1 - 3) / 2 + 1, s3 = (s2 - 3) / 2 + 1 (integer division; 64: 15 / 7 / 3):
 *        f1 = relu(conv(x; 3 -> 64, 11 x 11, stride 4, pad 2))            [64, s1, s1]
 *        f2 = relu(conv(maxpool(f1); 64 -> 192, 5 x 5, pad 2))            [192, s2, s2]
 *        f3 = relu(conv(maxpool(f2); 192 -> 384, 3 x 3, pad 1))           [384, s3, s3]
 *        f4 = relu(conv(f3; 384 -> 256, 3 x 3, pad 1)),  f5 = relu(conv(f4; 256 -> 256, 3 x 3, pad 1))
 *      maxpool = MaxPool2d(3, stride 2) without padding.
 *   6. per layer k and position p:  n(f) = f / (sqrt(sum_c f_c^2) + 1e-10),   d_k = mean_p sum_c w_kc (n(fa)_c - n(fb)_c)^2, w_k = lin{k}.
 *   7. lpips = d_1 + ... + d_5.
 * out [B] (device fp64): lpips.  layers_out: NULL, or device fp64 [B,5] that receives the d_k.
 * What is rounded to bf16 (round to nearest even): the convolution weights, the prepared input of step 4 and every stored activation
 * (each f_k after its ReLU, each max-pool output).  Biases, the lin weights and the scaling constants are fp32; the convolutions
 * accumulate in fp32; steps 1 - 4 and step 6 are fp32 arithmetic on those values; the sums over the positions of a layer and over the
 * layers are fp64.
 * The two images of a pair run through the same launches as faces f and B + f of one batch of 2B (input preparation, five convolutions
 * of the shared GEMM family, two max-pools), then one launch computes the per-workgroup fp64 partial sums of step 6 for all five layers
 * and a second, tiny one adds them in index order.  No atomics: equal inputs score exactly 0, swapping images and ref (same size, no
 * normalisation) keeps the bits, and a face has the same bits from call to call and at every slot of a batch of the same size (another
 * batch size may choose another GEMM tile).  The context owns its workspace per (batch, ref_res) and its launch program, rebuilt when a
 * pointer or flag changes; hd_num_ops / hd_debug_op_name / hd_debug_limit_ops / hd_debug_read_op (program 0) see it (the fp64 outputs of
 * the last two launches are read back as their 32-bit words).  The call enqueues on `stream`, only reads its inputs and does not
 * synchronise; the pointers must stay valid until that work is done.
 * HD_ERR_INVALID (HD_ERR_NOT_READY for weights that are not finalized), naming the argument and before any HIP call, for: a context of
 * another kind; batch outside [1, 1024]; res or ref_res not a multiple of 64 in [64, 512]; unit_range other than 0 or 1; a NULL images,
 * ref or out; images, ref, images_range or ref_range not aligned to 4 bytes, out or layers_out not to 8; out or layers_out overlapping an
 * input or each other, as byte ranges. */
int hd_lpips_create(hd_ctx** out, int device);
int hd_lpips(hd_ctx* ctx, int batch, const float* images, int res, const float* ref, int ref_res, int unit_range,
             const float* images_range, const float* ref_range, double* out, double* layers_out, void* stream);

/* Photo in, photo out: head boxes of uint8 photos become the reference's network input, and restored faces go back into the photos.
 * Every dataset class of the reference builds ln_face as  crop -> resize((32, 32), BICUBIC) -> resize((128, 128), BICUBIC) -> to_tensor
 * and the ground truth as  crop -> resize((128, 128), BICUBIC) -> to_tensor  (dataset_kface.py:86-98, infer_cr.py:53).  Both, and the
 * way back, are Pillow's 8-bit two-pass antialiased bicubic resize, which is integer arithmetic on float64 coefficients: results equal
 * Pillow's byte for byte (tests/golden/photo_pil.npz holds Pillow's own).  The rule, for one axis with `in` input and `out` output
 * samples, a = -0.5:
 *     scale = in / out (double);  fs = max(scale, 1);  support = 2 * fs;  ss = 1.0 / fs
 *     for xx in 0..out-1:
 *         center = (xx + 0.5) * scale
 *         xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), in)        (int) truncates
 *         k[x] = bicubic((x + xmin - center + 0.5) * ss)   for x in 0..xmax-xmin-1;   k[x] /= sum_x k[x] (added in index order)
 *         K[x] = (int)(k[x] * 2^22 + (k[x] < 0 ? -0.5 : 0.5))
 *         dst[xx] = clip8((sum_x src[xmin + x] * K[x] + 2^21) >> 22)                                          int32 sums
 *     bicubic(x): x = |x|;  x < 1: ((a + 2) x - (a + 3)) x x + 1;   x < 2: (((x - 5) x + 8) x - 4) a;   else 0
 *   All of k is float64 and no multiply is fused with an add (one fused multiply-add in bicubic or center moves a K by one).  A resize
 *   runs the horizontal pass first, into a uint8 intermediate (clipped and rounded), and the vertical pass on that; an axis whose size
 *   does not change is skipped, so a same-size resize is the identity.  The crop comes first: taps never leave the box.
 * photos [N,height,width,3] device uint8 (HWC, np.asarray of a PIL image); boxes [batch,4] HOST int32 (left, top, width, height), sides in
 * [1, 2048], inside the photo; photo_index [batch] HOST int32 in [0, N), or NULL (all 0).  The host arrays are read before the call
 * returns (they travel as launch arguments, 64 faces a launch).
 * hd_face_ingest: lr in [8, 64]: crop -> (lr, lr) -> (res, res), ln_face;  lr = 0: crop -> (res, res), the ground truth and what a real
 *   low-resolution crop needs.  res a multiple of 64 in [64, 512].  out [batch,3,res,res] device fp32 = byte / 255 (a true fp32 division,
 *   as to_tensor); out_u8: NULL, or device [batch,res,res,3] that receives the bytes.  workspace: device memory of at least
 *   hd_face_ingest_workspace(batch, lr, res) bytes (the (lr, lr) images; 0 and may be NULL with lr = 0).
 * hd_face_paste: faces [batch,3,res,res] device fp32; photos is updated in place.  Per face:
 *     q8 = clamp(floor(x * 255 + 0.5), 0, 255)          fp32, the multiply and the add rounded separately; NaN -> 0 (torchvision save_image)
 *     q  = resize of q8 to (width, height) of the box by the rule above
 *     d  = min(x, width - 1 - x, y, height - 1 - y);   m = 256 if feather == 0 else min(256, ((2 d + 1) * 256) / (2 feather))   (integers)
 *     photo = (photo * (256 - m) + q * m + 128) >> 8
 *   Bytes outside every box are not written.  Two boxes of one call that share a pixel of one photo are refused (boxes that touch are
 *   fine), so no result depends on an order.  feather in [0, 256].  workspace: at least hd_face_paste_workspace(batch, res) bytes (q8).
 * One kernel does every resize: a workgroup owns a band of output rows and columns of one face, computes the K of its rows and columns
 * in fp64 into LDS, runs the horizontal pass over the source rows the band needs into LDS and the vertical pass from there.  Only integers
 * depend on the banding: a face's bytes do not depend on its batch position, on the other faces or on the tiling.  Launches per call:
 * ceil(batch / 64) per resize (ingest: two resizes with lr > 0, else one; paste: one, after one launch that makes q8).
 * Both calls need no context, allocate nothing and do not synchronise; they enqueue on `stream`; the workspace is the caller's, free to
 * reuse when the call's work on `stream` is done.  Errors are reported through hd_last_error(NULL).  HD_ERR_INVALID, naming the argument
 * and before any HIP call, for: a NULL photos, boxes, out, faces or (when its size is not 0) workspace; n_photos < 1; height or width
 * outside [1, 16384]; batch outside [1, 4096]; a box side outside [1, 2048]; a box outside its photo; a photo_index outside [0, N); lr
 * other than 0 or [8, 64]; res not a multiple of 64 in [64, 512]; feather outside [0, 256]; overlapping boxes (paste); out or faces not
 * aligned to 4 bytes; workspace_bytes too small.  The workspace queries return HD_ERR_INVALID for a batch, lr or res the calls refuse. */
int64_t hd_face_ingest_workspace(int batch, int lr, int res);
int hd_face_ingest(const uint8_t* photos, int n_photos, int height, int width, const int32_t* boxes, const int32_t* photo_index, int batch,
                   int lr, int res, float* out, uint8_t* out_u8, void* workspace, int64_t workspace_bytes, void* stream);
int64_t hd_face_paste_workspace(int batch, int res);
int hd_face_paste(uint8_t* photos, int n_photos, int height, int width, const float* faces, int res, const int32_t* boxes,
                  const int32_t* photo_index, int batch, int feather, void* workspace, int64_t workspace_bytes, void* stream);

/* Progress previews: the denoised estimate of the row a face last ran, as an output of the sampling loop (diffusers'
 * `pred_original_sample` / `callback_on_step_end`).
 * hd_preview_config(on = 1, every, snapshots): from the next hd_prepare* on -- at once, when a batch is prepared -- the context owns the
 * planes x0_preview [B,4,L,L], preview_rows [B] and preview_snaps [snapshots][B,4,L,L] (every >= 1, 0 <= snapshots <= 64; hd_debug_read
 * reads them under these names, the rows as their int32 bits), and every hd_sample* call (all seven loop entry points) ends the update of
 * row k of face f by storing
 *     p = clamp((x - c0*eps)/c1, +-c2)            the x0 of that row: the value a multistep schedule keeps as its history
 *     p = m * x0 + (1 - m) * known                for a face that carries a mask (hd_mask_faces), in this order: m == 1 gives x0 and
 *                                                 m == 0 gives known bit for bit; the history keeps the unblended x0
 * to the face's latest plane, with k as its row, and -- j = k - begin_f the row inside the face's own schedule (begin_f = 0 without
 * hd_sample_spans), when (j + 1) % every == 0 and s = (j + 1)/every - 1 < snapshots -- to snapshot plane s as well.  A held face (past its
 * end row, or an empty slot with start == end) writes nothing.  Nothing is rebuilt or recaptured by switching previews on or off or
 * changing their size ("graph_captures" does not move), and while they are off the step launches read and compute what they did without
 * this call: x_inout is bit for bit the same either way.  on = 0 frees the planes.  The configuration survives hd_prepare*; like the
 * masks, every hd_prepare* resets all faces (row -1, zeroed planes), hd_prepare_slots the slots it refills, hd_preview_config(on = 1)
 * itself all faces, and hd_sample* calls never do: a loop split over calls keeps its previews.  hd_get_option "preview" returns `on`.
 * hd_eps and hd_scheduler_step* know no preview.  If a persistent stage gives up during a call (hd_check), the previews that call wrote
 * are unspecified.  The call synchronises the device (not for the hot path).  HD_ERR_INVALID on a CoarseRestoration / VAE context, for
 * every < 1, snapshots outside [0, 64] or on outside {0, 1}.
 * hd_preview_read: copy, in stream order, the latest plane (snapshot == -1) or snapshot plane `snapshot` of faces slots[j] (host [n],
 * distinct, in [0, B); NULL: n == B, faces in order) to x0_out [n,4,L,L] (device fp32), and to rows_out [n] (device int32, or NULL) the
 * table row of that estimate: for a snapshot plane begin_f + (snapshot + 1)*every - 1; -1 when the face has not written the plane since it
 * was prepared or refilled (its plane is then zero).  HD_ERR_NOT_READY without a prepared batch or with previews off; HD_ERR_INVALID for a
 * duplicate or out-of-range slot, n outside [1, B], slots == NULL with n != B, or snapshot outside [-1, snapshots). */
int hd_preview_config(hd_ctx* ctx, int on, int every, int snapshots);
int hd_preview_read(hd_ctx* ctx, int n, const int32_t* slots, int snapshot, float* x0_out, int32_t* rows_out, void* stream);

/* One scheduler update on its own: `scheduler.step(eps, t, x).prev_sample` (test_refiner.py:91) in
 * the coefficient form of hd_schedule (coef7 on the host); x updated in place.  noise/seed/step as in
 * hd_sample.  Needs no context. */
int hd_scheduler_step(float* x_inout, const float* eps, const float* coef7, const float* noise,
                      uint64_t seed, int step, int64_t n_elems, void* stream);
/* One multistep update (coef8 on the host, hd_schedule_ms form): x0_hist [n_elems] device fp32 is read for the c[7] term and
 * then overwritten with this step's x0.  x0_hist may be NULL only when c[7] == 0 (HD_ERR_INVALID otherwise). */
int hd_scheduler_step_multistep(float* x_inout, const float* eps, const float* coef8, float* x0_hist, const float* noise,
                                uint64_t seed, int step, int64_t n_elems, void* stream);

/* Introspection for tests and profiling (not on the hot path; reads synchronise the device).
 * `which` selects the launch program: 0 = one denoiser evaluation (hd_eps / one hd_sample step),
 * 1 = the most recent hd_prepare prologue. */
int hd_num_ops(hd_ctx* ctx, int which);                    /* kernel launches in the program (one chain) */
int hd_num_chains(hd_ctx* ctx);                            /* concurrently scheduled sub-batches       */
int hd_debug_limit_ops(hd_ctx* ctx, int which, int n_ops); /* run only the first n ops (<0: all)      */
const char* hd_debug_op_name(hd_ctx* ctx, int which, int i);
/* How launch i is dispatched.  0 for a launch that is not one of the shared GEMM kernels; otherwise
 *   bits 0-7   loader kind + 1    (0 F32, 1 LN, 2 BF16, 3 BF16S, 4 CONV_F32, 5 CONV_F32G, 6 CONV_BF16)
 *   bits 8-15  epilogue kind + 1  (0 BIASF32, 1 RESID, 2 GATE, 3 PIXSHUF, 4 BIASBF16, 5 DWGATE, 6 SCA)
 *   bits 16-23 kernel mode + 1    (0 / 1 tall 128 / 64 rows, 2 / 3 skinny 64 / 32 rows, 4 tall 32 rows x 256 columns, 5 / 6 skinny with
 *                                  128 / 256-row M-split workgroups; + 16 deep-prefetch tall kernel, + 32 role-split wide kernel) -- the
 *                                  mode the launch is given after the caller's hint and the HD_GEMM_MODE / HD_OP_MODE overrides
 *   bit 24     xcd_tile_affine (the workgroups of an XCD share weight tiles), bit 25 w_nt (non-temporal weight loads)
 * Negative: HD_ERR_INVALID (no such launch). */
int hd_debug_op_info(hd_ctx* ctx, int which, int i);
/* copy the output buffer of op i to the host as fp32; host_out NULL -> just return the element count */
int64_t hd_debug_read_op(hd_ctx* ctx, int which, int i, float* host_out, int64_t max_elems);
/* copy a named internal buffer (DESIGN.md "Buffers") to the host as fp32; returns the element count */
int64_t hd_debug_read(hd_ctx* ctx, const char* name, float* host_out, int64_t max_elems);
/* overwrite a named internal buffer from host fp32 (bf16 buffers: rounded to nearest even): tests feed a launch the
 * oracle's value of its input ("teacher forcing") so that its own error is not buried under inherited drift */
int hd_debug_write(hd_ctx* ctx, const char* name, const float* host_in, int64_t n_elems);
/* One launch of the shared GEMM kernels on the caller's operands (tests: a GEMM needs no network around it).  `ctx` is a context that
 * has been created but NOT finalized; `weight` names a pair <weight>.weight [N][K] (or [N][K][1][1]) / <weight>.bias [N] given to
 * hd_load_weights, packed on first use and cached in the context (PixelShuffle r = 2: the sub-pixel-major packing).  `loader` /
 * `epilogue` are the kinds of hd_debug_op_info (not + 1); the pairs the library builds without face geometry are accepted: F32 ->
 * BIASF32 / PIXSHUF, BF16 -> RESID / BIASBF16 / PIXSHUF / BIASF32, BF16S -> RESID, LN -> GATE / BIASF32.  The launch goes through the
 * library's own launch builder: kernel mode, deep / wide kernel, xcd_tile_affine and w_nt are chosen as for a launch of a program, so
 * every kernel this entry can start is one some program starts for some batch.  Nothing is allocated per call: every pointer of the
 * descriptor is a DEVICE pointer the caller owns, 16-byte aligned, NULL where the pair does not read it or the output is not wanted.
 *   A [M][lda]: fp32 (F32) or bf16 (others); a_scale: F32 only.  BF16S: rowscale [M / hw][K].  LN: stats_in [M][stats_np] (mean, M2)
 *   partials of stats_cnt elements each, film + film_gain_off / film_bias_off [K] fp32 (film_face_stride != 0: the row of face
 *   face0 + row / hw at that stride, the per-face kernel), ln_eps 1e-6.
 *   out [M][ldo]: fp32, or bf16 for GATE ([M][N / 2]) and BIASBF16; out16 (bf16 copy, same ld) and stats_out [M][N / 32] (mean, M2)
 *   for the fp32 epilogues.  RESID: resid fp32 [M][ldr], rscale [N], and with outg16 also gate_c [M / hw][N], gate_s [M], add_src
 *   ([M][ldo] or NULL).  BIASBF16: resid bf16 [M][ldr] or NULL.  PIXSHUF: no bias; resid (or NULL) in the layout of out;
 *   shuffle_r = 2: rows are pixels of Win x Win images, out [4 M][ldo] with ldo = N / 4.  act: 0 none, 1 ReLU, 2 sigmoid (BIASF32, BIASBF16).
 * HD_ERR_INVALID with a message that names the field, before any launch, for: a finalized context, an unknown weight, a pair outside
 * the list, K % 8 != 0, lda < K, a pointer the pair reads that is NULL or not 16-byte aligned, stats_np * stats_cnt != K, M % hw != 0
 * where rows are mapped to faces, PixelShuffle r = 2 with Win or ldo not a power of two or M % Win^2 != 0, and leading dimensions the
 * kernels cannot address.  `note` receives what the launchers started (zero for a dry run) and the hd_debug_op_info word of the op.
 * flags: HD_GEMM_DRY_RUN = build the op, return its word, launch nothing. */
typedef struct hd_gemm_desc {
    int32_t M, hw, face0, act, shuffle_r, Win, stats_np, stats_cnt;
    float a_scale;
    int32_t film_face_stride, film_gain_off, film_bias_off;
    int32_t lda, ldo, ldr;
    int32_t reserved;
    const void* A;
    const float* stats_in;
    const float* film;
    const float* rowscale;
    const void* resid;
    const float* rscale;
    const float* gate_c;
    const float* gate_s;
    const float* add_src;
    void* out;
    void* out16;
    void* outg16;
    float* stats_out;
} hd_gemm_desc;
typedef struct hd_gemm_note {
    int32_t op_info;        /* as hd_debug_op_info */
    int32_t family;         /* 1 tall, 2 deep-prefetch tall, 3 skinny, 4 wide; 0: nothing was launched */
    int32_t rows;           /* rows per workgroup */
    int32_t pair;           /* both gate halves in one workgroup */
    int32_t wk, cpw, nt;    /* skinny: waves along K, chunks per wave of the straight-line K loop (0: the run-time loop), non-temporal weights */
    int32_t wide_form;      /* wide: 1 (128 rows), 2 (256), 3 (64) */
    int32_t threads;
    int32_t grid_x, grid_y;
} hd_gemm_note;
enum { HD_GEMM_DRY_RUN = 1 };
int hd_debug_gemm(hd_ctx* ctx, const char* weight, int loader, int epilogue, const hd_gemm_desc* desc, int flags, hd_gemm_note* note,
                  void* stream);
/* One launch of a face-geometry convolution on the caller's operands, through the builder the programs call (tests: the kernels whose
 * rows depend on their neighbours in the face, without a network around them).  `ctx` as for hd_debug_gemm: created, NOT finalized.
 *   HD_CONV_HCA:  the HCA 3x3 (pad 1) conv C -> C + bias, ReLU, through add_hca.  `weight` names <weight>.weight [C][C][3][3] and
 *                 <weight>.bias [C] (no BatchNorm is folded).  side == 1 packs the centre tap only, as the programs do for 1 x 1 faces.
 *                 X bf16 [M][C], rows are pixels of M / side^2 faces; out fp32 [M][C]; out16 bf16 copy or NULL; stats_out NULL.
 *   HD_CONV_DOWN: the 2x2 stride-2 down-conv C -> 2C + bias through add_down.  <weight>.weight [2C][C][2][2], <weight>.bias [2C].
 *                 X bf16 [M][C] (faces of side x side); out fp32 [M / 4][2C]; out16 and stats_out [M / 4][2C / 32] (mean, M2) or NULL.
 * The weight is packed on first use (pack_weight) and cached in the context.  The library picks the kernel from (C, side, M) as for a
 * launch of a program -- the LDS-staged conv for the (C, side) pairs of add_hca's table, the patch-gather GEMM otherwise -- and `note`
 * says what ran: form 1 = staged (the ConvCfg by its parameters, faces per workgroup, grid, and whether the kernel's XCD tile remap
 * applied to that grid), form 2 = patch-gather GEMM (`gemm` as hd_debug_gemm fills it); form 0 and gemm.op_info only after a dry run.
 *   HD_CONV_DWGATE: the front of a NAF block's attention half, LayerNorm + FiLM -> conv1 (+ bias) -> depthwise 3x3 (pad 1) on both halves
 *                 -> their product G (bf16) and its mean per face, through the function the block builder calls (add_conv1_dwgate).
 *                 `weight` names conv1 (<weight>.weight [2C][C] or [2C][C][1][1], .bias [2C]), `weight2` conv2 (<weight2>.weight
 *                 [2C][1][3][3], .bias [2C]).  X bf16 [M][C]; stats_in [M][stats_np] (mean, M2) partials of stats_cnt elements each;
 *                 film fp32 with the bias row at film_off and the gain row at film_off + C (film_face_stride != 0: the row of face
 *                 face0 + row / side^2 at that stride); G bf16 [M][C]; pooled fp32 [M / side^2][C]; pooled16 bf16 copy or NULL (the
 *                 fused form writes it); T1 fp32 scratch of T1_elems >= 2 M C + faces * ((side + 7) / 8) * C elements.  The library
 *                 picks the form from (C, side, M, stats_np) and note.dw_path says which: 1 fused into conv1's epilogue (`gemm` says
 *                 which kernel), 2 by strips (T1 then holds [face][side / 4][C] strip sums and pooled is NOT written: the chain kernel
 *                 adds them up), 3 unfused (T1 [M][2C] = conv1's output, band sums behind it, pooled by pool_finish).  dw_path is
 *                 filled by a dry run too.  out, out16 and stats_out are NULL.  side up to 64.
 * `weight2` is NULL for the other kinds.  Every pointer is a DEVICE pointer the caller owns.
 * HD_ERR_INVALID with a message that names the field, before any launch, for: a finalized context, an unknown kind, side not a power
 * of two (or > 32; DOWN: < 2), M < 1, M > 65536 or M % side^2 != 0, C not a multiple of 32 (or > 2048), a pointer that is NULL where it is needed
 * or not 16-byte aligned, stats_out with HD_CONV_HCA, and a weight or bias that is missing or whose shape does not match (C, kind).
 * The accepted range is that of the programs' levels (C = 128 .. 2048, faces up to 32 x 32) and of the tests: M * C <= 2^27, so every
 * index the loaders and epilogues form in 32 bits (row * C + c, K = 9 C) stays below 2^31.
 * flags: HD_GEMM_DRY_RUN as for hd_debug_gemm. */
typedef struct hd_conv_desc {
    int32_t M, C, side;
    int32_t face0, stats_np, stats_cnt, film_off, film_face_stride;     /* HD_CONV_DWGATE */
    int64_t T1_elems;
    const void* X;
    float* out;
    void* out16;
    float* stats_out;
    const float* stats_in;                                              /* HD_CONV_DWGATE from here on */
    const float* film;
    void* G;
    float* pooled;
    void* pooled16;
    float* T1;
} hd_conv_desc;
typedef struct hd_conv_note {
    int32_t form;           /* 1 staged in LDS (hd_conv.hpp), 2 patch-gather GEMM, 3 HD_CONV_DWGATE (see dw_path); 0: nothing was launched */
    int32_t centre_only;    /* the weight was packed with its centre tap only */
    int32_t C, side;        /* staged: the ConvCfg that ran ... */
    int32_t bm, mt, ks, nt, strip, depth;
    int32_t faces_per_wg;   /* ... whole faces per workgroup (1 where a face is one or more workgroups) */
    int32_t threads, grid_x, grid_y;
    int32_t remap;          /* staged: the XCD tile remap's condition held for this grid */
    int32_t hint;           /* gather: the kernel mode the builder asked add_gemm for (-1: none) */
    int32_t dw_path;        /* HD_CONV_DWGATE: 1 fused, 2 by strips, 3 unfused (also after a dry run) */
    hd_gemm_note gemm;      /* gather: as hd_debug_gemm */
} hd_conv_note;
enum { HD_CONV_HCA = 0, HD_CONV_DOWN = 1, HD_CONV_DWGATE = 2 };
int hd_debug_conv(hd_ctx* ctx, int kind, const char* weight, const char* weight2, const hd_conv_desc* desc, int flags, hd_conv_note* note,
                  void* stream);
/* Run-time switches that select between equivalent launch programs of the same arithmetic (tests compare them bit for
 * bit; no reference interface corresponds): "xcd" 1/0 = levels 2 / 3 as XCD-local persistent launches (hd_xcd.hpp) or one
 * launch per GEMM; "face" 1/0 the same for levels 0 / 1 (hd_face.hpp); "xcd_phase_limit" n / "face_block_limit" n = stop
 * the persistent stages after n phases / blocks (0: all), "stage_limit_first" i = only the stage whose first block has index
 * i (-1: every stage) -- tests read a stage's residual stream block by block; "xcd_force_global" 1 = its
 * placement-independent hand-off form.  hd_get_option: "xcd" (effective), "xcd_stages" (stages built so far);
 * "sample_stage_launches" / "sample_face_stage_launches" / "rows_stage_launches": persistent-stage launches (all / face-cluster only) that
 * the last one-step capture of hd_sample* / hd_sample_rows* recorded (-1 before the first capture; a stage that fell back is not counted);
 * "graph_captures": step graphs instantiated by this context so far (hd_prepare_slots and hd_mask_faces add none); "masked_faces": faces
 * of the batch that carry a mask (hd_mask_faces; hd_debug_read names "mask", "mask_known", "mask_noise" read the batch's mask buffers). */
int hd_set_option(hd_ctx* ctx, const char* key, int value);
int hd_get_option(hd_ctx* ctx, const char* key);
/* Error status of the asynchronous calls.  hd_eps / hd_sample only enqueue work; a persistent stage launch that has to give
 * up a hand-off wait (a workgroup of the stage was not resident: another tenant on the GPU) fills THAT call's result
 * (eps_out / x_inout) with NaN on the device and raises a host-visible word.  hd_check() -- to be called after the caller
 * has synchronised the stream, e.g. where the reference's loop would have raised RuntimeError (test_refiner.py:89-91) --
 * returns HD_ERR_HIP once for such a call (hd_last_error() names the stage and phase) and switches the context to one
 * launch per GEMM; the next hd_eps / hd_sample performs the same check on entry.  0 when nothing failed.
 * Fault injection for tests: hd_set_option(ctx, "stage_test_abort", n): n in 1..: group 0 of every XCD-local stage gives up
 * its wait for phase n - 1; 1000 + b: face 0 of every face-cluster stage gives up the pool wait of block b; 2000 + p: the first
 * loader wave of group 0 of every autonomous-wave stage (hd_xcd2.hpp) gives up its wait before LayerNorm phase p (p = 0 or 3 mod 5);
 * 0: off.  Every call issued between a stage giving up and the check that reports it may be NaN-poisoned: the report names the
 * first failure only. */
int hd_check(hd_ctx* ctx);
/* HIP-event time in ms of the most recent hd_sample's replay loop (0 if profiling is off) and the
 * summed duration of the GEMM launches: used by bench.py for the roofline object */
int hd_set_profiling(hd_ctx* ctx, int on);
int hd_get_profile(hd_ctx* ctx, double* loop_ms, double* step_ms_avg, int64_t* weight_bytes_per_step,
                   double* flops_per_face_step);

#ifdef __cplusplus
}
#endif
#endif /* HIFIDIFF_HIP_H */
