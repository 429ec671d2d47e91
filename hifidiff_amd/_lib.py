"""ctypes binding of libhifidiff_hip.so (C-ABI: include/hifidiff_hip.h) and its in-tree build.

There is no CPU fallback: if the shared library is missing or no gfx950 device is present, every
entry point raises.  Build with `python -c "import __graft_entry__ as g; g.build()"` (hipcc
cross-compiles for gfx950 without a GPU).
"""
import ctypes
import os
import subprocess

# PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  It must be loaded BEFORE this
# library so that our DT_NEEDED libamdhip64.so.7 resolves to that same runtime instance: one HIP runtime
# per process, shared streams and allocations.  Loading ours first pulls in /opt/rocm's copy and the
# process ends up with two runtimes (torch then reports "No HIP GPUs are available").
import torch  # noqa: F401  (load order matters, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhifidiff_hip.so")
# translation units (compiled in parallel, one hipcc each) and the headers they include
UNITS = [os.path.join(_HERE, "csrc", f) for f in ("hd_lib.hip", "hd_aux.hip", "hd_stages.hip", "hd_stages_rows.hip", "hd_strip.hip", "hd_dispatch_ln.hip", "hd_dispatch_lnface.hip", "hd_dispatch_bf16.hip", "hd_dispatch_misc.hip", "hd_lpips.hip", "hd_photo.hip", "hd_image.hip")]
SOURCES = UNITS + [os.path.join(_HERE, "csrc", f) for f in ("hd_gemm.hpp", "hd_dispatch.hpp", "hd_kernels.hpp", "hd_chain.hpp", "hd_conv.hpp", "hd_cr.hpp", "hd_vae.hpp", "hd_internal.hpp", "hd_faceset.hpp", "hd_stage_api.hpp", "hd_xcd.hpp", "hd_xcd2.hpp", "hd_face.hpp", "hd_strip.hpp", "hd_wide.hpp", "hd_end.hpp", "hd_color.hpp", "hd_metrics.hpp", "hd_lpips.hpp", "hd_photo.hpp", "hd_args.hpp", "hd_bicubic.hpp")]
HEADER = os.path.join(os.path.dirname(_HERE), "include", "hifidiff_hip.h")


def unit_deps(unit):
    """The unit and every file it includes with #include "..." (recursively): what its object file depends on."""
    import re
    seen, todo = [], [unit]
    while todo:
        f = os.path.normpath(todo.pop())
        if f in seen or not os.path.exists(f):
            continue
        seen.append(f)
        with open(f) as fh:
            for inc in re.findall(r'^\s*#include\s+"([^"]+)"', fh.read(), flags=re.M):
                todo.append(os.path.join(os.path.dirname(f), inc))
    return seen

EXPORTS = [
    "hd_create", "hd_create_unconditional", "hd_prepare_unconditional", "hd_cr_create", "hd_cr_forward", "hd_vae_create", "hd_vae_encode", "hd_vae_decode", "hd_destroy", "hd_last_error", "hd_load_weights", "hd_finalize_weights", "hd_prepare",
    "hd_prepare_from_priors", "hd_fpg", "hd_idc", "hd_eps", "hd_sample", "hd_sample_multistep", "hd_sample_rows", "hd_sample_rows_multistep", "hd_prepare_slots",
    "hd_pool_config", "hd_pool_prepare", "hd_pool_commit",
    "hd_sample_faces", "hd_sample_faces_multistep", "hd_sample_spans", "hd_mask_faces", "hd_guide_config", "hd_guide_faces", "hd_color_fix", "hd_image_range", "hd_image_metrics", "hd_image_metrics_workspace", "hd_lpips_create", "hd_lpips", "hd_face_ingest", "hd_face_ingest_workspace", "hd_face_paste", "hd_face_paste_workspace", "hd_preview_config", "hd_preview_read", "hd_scheduler_step",
    "hd_scheduler_step_multistep", "hd_num_ops", "hd_num_chains",
    "hd_debug_limit_ops", "hd_debug_op_name", "hd_debug_op_info", "hd_debug_read_op", "hd_debug_read", "hd_debug_write", "hd_debug_gemm", "hd_debug_conv", "hd_set_option", "hd_get_option", "hd_check",
    "hd_set_profiling", "hd_get_profile",
]


class TensorDesc(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("ndim", ctypes.c_int32),
                ("shape", ctypes.c_int64 * 4), ("is_device", ctypes.c_int32)]


class Schedule(ctypes.Structure):
    _fields_ = [("n_steps", ctypes.c_int32), ("timesteps", ctypes.POINTER(ctypes.c_float)),
                ("coef", ctypes.POINTER(ctypes.c_float))]


class ScheduleMS(ctypes.Structure):
    _fields_ = [("n_steps", ctypes.c_int32), ("timesteps", ctypes.POINTER(ctypes.c_float)),
                ("coef", ctypes.POINTER(ctypes.c_float))]


class GemmDesc(ctypes.Structure):
    """hd_gemm_desc: one GEMM launch on the caller's device buffers (hd_debug_gemm)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("M", "hw", "face0", "act", "shuffle_r", "Win", "stats_np", "stats_cnt")] + [("a_scale", ctypes.c_float)] + \
               [(n, ctypes.c_int32) for n in ("film_face_stride", "film_gain_off", "film_bias_off", "lda", "ldo", "ldr", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("A", "stats_in", "film", "rowscale", "resid", "rscale", "gate_c", "gate_s", "add_src", "out", "out16", "outg16", "stats_out")]


class GemmNote(ctypes.Structure):
    """hd_gemm_note: the hd_debug_op_info word of the op and what the launchers started."""
    _fields_ = [(n, ctypes.c_int32) for n in ("op_info", "family", "rows", "pair", "wk", "cpw", "nt", "wide_form", "threads", "grid_x", "grid_y")]


GEMM_DRY_RUN = 1


class ConvDesc(ctypes.Structure):
    """hd_conv_desc: one face-geometry convolution on the caller's device buffers (hd_debug_conv)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("M", "C", "side", "face0", "stats_np", "stats_cnt", "film_off", "film_face_stride")] + \
               [("T1_elems", ctypes.c_int64)] + \
               [(n, ctypes.c_void_p) for n in ("X", "out", "out16", "stats_out", "stats_in", "film", "G", "pooled", "pooled16", "T1")]


class ConvNote(ctypes.Structure):
    """hd_conv_note: which kernel hd_debug_conv's builder started (form 1: staged in LDS, 2: patch-gather GEMM) and its shape."""
    _fields_ = [(n, ctypes.c_int32) for n in ("form", "centre_only", "C", "side", "bm", "mt", "ks", "nt", "strip", "depth", "faces_per_wg", "threads",
                                              "grid_x", "grid_y", "remap", "hint", "dw_path")] + [("gemm", GemmNote)]


CONV_HCA, CONV_DOWN, CONV_DWGATE = 0, 1, 2


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -shared: compiles every HIP kernel of the path into the in-tree .so."""
    if not force and os.path.exists(LIB_PATH):
        newest = max(os.path.getmtime(p) for p in SOURCES + [HEADER])
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-function"]
    objdir = os.path.join(_HERE, "csrc", "build")
    os.makedirs(objdir, exist_ok=True)
    objs = [os.path.join(objdir, os.path.splitext(os.path.basename(u))[0] + ".o") for u in UNITS]
    # a unit is recompiled when it or a header it includes is newer than its object file
    stale = [(u, o) for u, o in zip(UNITS, objs)
             if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(d) for d in unit_deps(u))]
    cmds = [[hipcc] + flags + ["-c", u, "-o", o] for u, o in stale]
    if verbose:
        for c in cmds:
            print(" ".join(c))
    procs = [subprocess.Popen(c) for c in cmds]                 # the kernel instantiations dominate: one process per unit
    failed = [u for (u, _), pr in zip(stale, procs) if pr.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, "hipcc -c " + " ".join(os.path.basename(f) for f in failed))
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(link))
    subprocess.run(link, check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is not built (no CPU fallback exists); run __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    L.hd_create.argtypes = [ctypes.POINTER(vp), i32, i32]
    L.hd_create_unconditional.argtypes = [ctypes.POINTER(vp), i32, i32]
    L.hd_prepare_unconditional.argtypes = [vp, i32, vp]
    L.hd_cr_create.argtypes = [ctypes.POINTER(vp), i32]
    L.hd_cr_forward.argtypes = [vp, i32, vp, vp, vp]
    L.hd_vae_create.argtypes = [ctypes.POINTER(vp), i32]
    L.hd_vae_encode.argtypes = [vp, i32, i32, i32, vp, i32, vp, u64, vp, vp, vp]
    L.hd_vae_decode.argtypes = [vp, i32, i32, vp, vp, vp]
    L.hd_destroy.argtypes = [vp]; L.hd_destroy.restype = None
    L.hd_last_error.argtypes = [vp]; L.hd_last_error.restype = ctypes.c_char_p
    L.hd_load_weights.argtypes = [vp, ctypes.POINTER(TensorDesc), i32]
    L.hd_finalize_weights.argtypes = [vp]
    L.hd_prepare.argtypes = [vp, i32, vp, vp, vp, vp]
    L.hd_prepare_from_priors.argtypes = [vp, i32, ctypes.POINTER(vp), vp, vp]
    L.hd_fpg.argtypes = [vp, i32, vp, ctypes.POINTER(vp), vp]
    L.hd_idc.argtypes = [vp, i32, vp, vp, vp]
    L.hd_eps.argtypes = [vp, vp, vp, i32, vp, vp]
    L.hd_sample.argtypes = [vp, vp, ctypes.POINTER(Schedule), vp, u64, vp]
    L.hd_scheduler_step.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float), vp, u64, i32, i64, vp]
    L.hd_sample_multistep.argtypes = [vp, vp, ctypes.POINTER(ScheduleMS), vp, u64, vp]
    L.hd_sample_rows.argtypes = [vp, vp, ctypes.POINTER(Schedule), vp, i32, vp, u64, vp]
    L.hd_sample_rows_multistep.argtypes = [vp, vp, ctypes.POINTER(ScheduleMS), vp, i32, i32, vp, u64, vp]
    L.hd_prepare_slots.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int32), vp, vp, vp, vp]
    L.hd_pool_config.argtypes = [vp, i32]
    L.hd_pool_prepare.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int32), vp, vp, vp, vp]
    L.hd_pool_commit.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), vp]
    L.hd_sample_faces.argtypes = [vp, vp, ctypes.POINTER(Schedule), ctypes.POINTER(ctypes.c_int32), i32, ctypes.POINTER(u64), vp, u64, vp]
    L.hd_sample_faces_multistep.argtypes = [vp, vp, ctypes.POINTER(ScheduleMS), ctypes.POINTER(ctypes.c_int32), i32, ctypes.POINTER(ctypes.c_int32),
                                            ctypes.POINTER(u64), vp, u64, vp]
    L.hd_sample_spans.argtypes = [vp, vp, ctypes.POINTER(ScheduleMS), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                  ctypes.POINTER(ctypes.c_int32), i32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(u64), vp, u64, vp]
    L.hd_mask_faces.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int32), vp, vp, vp, vp]
    L.hd_guide_config.argtypes = [vp, i32]
    L.hd_guide_faces.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int32), vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32),
                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), vp]
    L.hd_color_fix.argtypes = [vp, vp, i32, i32, vp, i32, i32, i32, i32, vp, vp]
    L.hd_image_range.argtypes = [vp, i32, i32, i32, vp, vp]
    L.hd_image_metrics.argtypes = [vp, i32, vp, i32, i32, i32, ctypes.c_float, vp, vp, vp, vp, vp, i64, vp]
    L.hd_image_metrics_workspace.argtypes = [i32, i32, i32]; L.hd_image_metrics_workspace.restype = i64
    L.hd_lpips_create.argtypes = [ctypes.POINTER(vp), i32]
    L.hd_lpips.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    L.hd_face_ingest_workspace.argtypes = [i32, i32, i32]; L.hd_face_ingest_workspace.restype = i64
    L.hd_face_ingest.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, i64, vp]
    L.hd_face_paste_workspace.argtypes = [i32, i32]; L.hd_face_paste_workspace.restype = i64
    L.hd_face_paste.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, vp, i64, vp]
    L.hd_preview_config.argtypes = [vp, i32, i32, i32]
    L.hd_preview_read.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_int32), i32, vp, vp, vp]
    L.hd_scheduler_step_multistep.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float), vp, vp, u64, i32, i64, vp]
    L.hd_num_ops.argtypes = [vp, i32]
    L.hd_num_chains.argtypes = [vp]
    L.hd_debug_limit_ops.argtypes = [vp, i32, i32]
    L.hd_debug_op_name.argtypes = [vp, i32, i32]; L.hd_debug_op_name.restype = ctypes.c_char_p
    L.hd_debug_op_info.argtypes = [vp, i32, i32]
    L.hd_debug_read_op.argtypes = [vp, i32, i32, vp, i64]; L.hd_debug_read_op.restype = i64
    L.hd_debug_read.argtypes = [vp, ctypes.c_char_p, vp, i64]; L.hd_debug_read.restype = i64
    L.hd_debug_write.argtypes = [vp, ctypes.c_char_p, vp, i64]
    L.hd_debug_gemm.argtypes = [vp, ctypes.c_char_p, i32, i32, ctypes.POINTER(GemmDesc), i32, ctypes.POINTER(GemmNote), vp]
    L.hd_debug_conv.argtypes = [vp, i32, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ConvDesc), i32, ctypes.POINTER(ConvNote), vp]
    L.hd_set_option.argtypes = [vp, ctypes.c_char_p, i32]
    L.hd_get_option.argtypes = [vp, ctypes.c_char_p]
    L.hd_check.argtypes = [vp]
    L.hd_set_profiling.argtypes = [vp, i32]
    L.hd_get_profile.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double)]
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int and name not in ("hd_num_ops",):
            fn.restype = ctypes.c_int
    _lib = L
    return L


class HipError(RuntimeError):
    pass


def check(rc, ctx=None):
    """Negative return -> RuntimeError(hd_last_error()), like the reference raising on bad shapes."""
    if rc is not None and rc < 0:
        msg = lib().hd_last_error(ctx)
        raise HipError(f"hifidiff_hip error {rc}: {msg.decode() if msg else '?'}")
    return rc
