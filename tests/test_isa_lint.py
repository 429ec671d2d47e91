"""ISA lint of the in-tree gfx950 build (CPU: hipcc cross-compiles; llvm-objdump / llvm-readelf read the code objects that
__graft_entry__.build() made).  VERDICT r03 #5: what was a 300x GPU lottery becomes a build-time guard --
  (i)   no `scratch_` instruction (register spill) in the persistent stage kernels, the chain kernels and the skinny-GEMM
        instantiations the benchmark's step launches (one FiLM row for all faces: LdF32LN_T<false>, and the plain loaders);
  (ii)  no `flat_` instruction anywhere (a generic pointer costs `s_waitcnt vmcnt(0) lgkmcnt(0)` inside K loops);
  (iii) no packed-fp32 VALU instruction with `op_sel:[0,1,0] op_sel_hi:[1,1,0]` -- the operand form that
        profiles/r03_unit_stats_isa/ isolated as the one producing launch-to-launch differences in the LayerNorm transform
        (utils.py:16-24 is the arithmetic concerned) -- in ANY kernel, hd_face.hpp / hd_chain.hpp / hd_xcd2.hpp included.
The per-kernel table goes to profiles/r04_isa_report.txt (tools/isa_report.py)."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recs():
    import __graft_entry__ as g
    import isa_report
    g.build()                                             # no-op when the .so is newer than the sources
    if not os.path.isdir(isa_report.BUILD) or not [f for f in os.listdir(isa_report.BUILD) if f.endswith(".o")]:
        pytest.skip("object files of the in-tree build are not present (prebuilt .so only)")
    return isa_report.collect()


def _p(r):
    return r["pretty"].replace("void ", "").replace("hd::", "")


# the stage instantiations the benchmark's 59-launch step runs (latent 16, batch <= 64): level 0 / 1 face clusters, level 2 in the
# autonomous-wave form, level 3 in the K-split form.  The other instantiations (xcd_stage<512,16>: 3 spilled registers,
# naf_face_stage<256,32>: 30, xcd2<1024,4>) are the forms hd_set_option / HD_XCD2 / HD_FACE_L1_ROWS select; <256,32> has no down-conv
# entry, so that form runs downs.0 as a launch of its own (tests/test_program_variants.py).
BENCH_STAGES = ("xcd_stage_kernel<1024, 4>", "xcd2_stage_kernel<512, 16>", "naf_face_stage_kernel<128, 32>", "naf_face_stage_kernel<256, 16>")


def test_no_scratch_in_the_hot_kernels(recs):
    stages = [r for r in recs if _p(r).startswith(BENCH_STAGES)]
    assert len(stages) == len(BENCH_STAGES), [_p(r)[:60] for r in stages]
    bad = [(_p(r)[:80], r["scratch"], r["vgpr_spill"], r["scratch_bytes"]) for r in stages if r["scratch"] or r["vgpr_spill"] or r["scratch_bytes"]]
    assert not bad, bad
    # the step's last launch (hd_end.hpp: the last HCA conv + the ending conv): one copy per translation unit that includes it
    ends = [r for r in recs if _p(r).startswith("hca_ending_conv_kernel")]
    assert ends and not [r for r in ends if r["scratch"] or r["vgpr_spill"] or r["scratch_bytes"]], [(_p(r)[:60], r["scratch"]) for r in ends]
    # latent 32, level 0 by strips (hd_strip.hpp); the level-1 form (C = 256) carries 12 spilled registers around an MFMA / VALU overlap
    strips = [r for r in recs if _p(r).startswith("naf_strip_dwgate_kernel<128, 32>")]
    assert len(strips) == 1 and not (strips[0]["scratch"] or strips[0]["vgpr_spill"]), [(_p(r)[:60], r["scratch"]) for r in strips]
    chains = [r for r in recs if _p(r).startswith("naf_chain_kernel")]
    assert len(chains) >= 3
    bad = [(_p(r)[:80], r["scratch"]) for r in chains if r["scratch"] or r["vgpr_spill"]]
    assert not bad, bad
    # the skinny GEMMs of the benchmark step: everything except the per-face-timestep LayerNorm loader (LdF32LN_T<true>,
    # used only when faces carry different timesteps -- not in the sampling loop)
    skinny = [r for r in recs if _p(r).startswith("gemm_skinny_kernel") and "LdF32LN_T<true>" not in _p(r)]
    assert len(skinny) > 50
    bad = [(_p(r)[:120], r["scratch"]) for r in skinny if r["scratch"] or r["vgpr_spill"]]
    assert not bad, bad


def test_no_flat_instructions(recs):
    bad = [(_p(r)[:100], r["flat"]) for r in recs if r["flat"]]
    assert not bad, bad


def test_no_packed_fp32_with_the_unreproducible_operand_form(recs):
    assert sum(r["pk_f32"] for r in recs) > 10000          # the scan sees the packed instructions at all
    bad = [(_p(r)[:100], r["bad_opsel"]) for r in recs if r["bad_opsel"]]
    assert not bad, bad
