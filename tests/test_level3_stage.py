"""The level-3 XCD-local stages (hd_xcd.hpp <1024, 4>: the 8-block encoder and the 2-block decoder of the default program) on
their own, block by block against the oracle, at batch 2 and at the benchmark batch.  Their bit-for-bit agreement with the per-GEMM
launches is tests/test_gpu_parity.py's job; this file holds the level-3 rows of the stage scan to the same bounds as
test_persistent_stages_block_by_block_against_oracle and also checks that every block of both stages is present in the scan."""
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

ROW = re.compile(r"^\s*\d+ (denoiser\.(encoders\.3|decoders\.0)\.(\d+)) \(stage\)\s+(X|X'-X)\s+rel (\S+)")


def level3_rows(report):
    """(block name, quantity, rel) of the level-3 stage rows of a stage scan report."""
    out = []
    for r in report:
        m = ROW.match(r)
        if m:
            out.append((m.group(1), m.group(4), float(m.group(5))))
    return out


@pytest.fixture(scope="module")
def model16(weights16):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    from hifidiff_amd.refiner import FacialRefiner
    m = FacialRefiner(16)
    m.load_state_dict(weights16)
    m.to("cuda:0")
    return m


@pytest.mark.parametrize("B", [2, 64])
def test_level3_stages_block_by_block_against_oracle(model16, weights16, B):
    import op_forced
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(B, 16)
    rep = []
    op_forced.stage_forced_scan(model16, weights16, x, crl, crf, 500.0, rep)
    rows = level3_rows(rep)
    names = sorted({n for n, _, _ in rows})
    want = sorted([f"denoiser.encoders.3.{b}" for b in range(8)] + [f"denoiser.decoders.0.{b}" for b in range(2)])
    assert names == want, names
    assert len(rows) == 2 * len(want), rows
    for n, what, rel in rows:
        lim = 3e-4 if what == "X" else 3e-3                    # fp32 output / the block's contribution through bf16 tiles
        assert rel <= lim, (B, n, what, rel)
