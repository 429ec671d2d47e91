"""The NAF block rules of the teacher-forced scans (tools/forced.py: NafRules) restate the oracle -- without a GPU.

One block is run on the CPU oracle with taps; the taps are handed to the rule set as if they had been read back from the device
(G and G2 rounded to bf16 as the kernels store them, the pooled mean and its bf16 copy, the bf16 copies and float64 (mean, M2)
LayerNorm partials next to conv3 / conv5), launch by launch, for every launch form of add_naf_block.  The rules then have to
reproduce the oracle exactly: every rel-L2 line 0.0, every bit-exact line 0 elements, the float64 and statistics lines within
their bounds, no launch without a rule.  The same feed with every launch's output scaled by 1.01 must flag every rel-L2 line
(1e-2 is above both bounds), so a rule that compares nothing cannot pass.
"""
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
sys.path.insert(0, os.path.join(ROOT, "tools"))
import forced                                                   # noqa: E402
from hifidiff_amd import arch, synth                            # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

B, C, P_ = 3, 64, "blk"                                        # C = 64: two 32-channel partials per row
FUSED = ["conv2_gate_pool", "sca", "conv3", "conv4", "conv5"]
UNFUSED = ["conv1", "conv2_gate_pool", "pool_finish", "sca", "conv3", "conv4", "conv5"]
CHAIN = ["conv2_gate_pool", "conv5"]                            # behind a fused conv1, or (C, H in STRIP_SHAPES) behind the strips
CHAIN_UNFUSED = ["conv1", "conv2_gate_pool", "pool_finish", "conv5"]


def _partials(vals, cnt=32):
    v = vals.double().reshape(vals.shape[0], -1, cnt)
    mean = v.mean(-1)
    return torch.stack((mean, (v - mean[..., None]).pow(2).sum(-1)), -1).float().reshape(-1)


@pytest.fixture(scope="module", params=[256, None], ids=["film", "plain"])
def block(request):
    """(weights, {H: (input, taps)}, the LayerNorm affine) of one block, conditional (time_dim 256) or plain."""
    torch.set_grad_enabled(False)
    manifest = {}
    arch._naf_block(manifest, P_, C, request.param)
    P = synth.make_state_dict(manifest)
    temb = torch.from_numpy(synth.randn("forced_rules/temb", (B, 256)))
    runs = {}
    for H in (4, 8):                                            # H * H <= 16: the sca launch rescales G in place; else conv3's loader does
        x = torch.from_numpy(synth.randn(f"forced_rules/x{H}", (B, C, H, H)))
        taps = {}
        if request.param:
            O.cond_naf_block(P, P_, x, temb, prec=O.BF16, taps=taps)
        else:
            O.naf_block(P, P_, x, prec=O.BF16, taps=taps)
        runs[H] = (x, {k[len(P_) + 1:]: v for k, v in taps.items()})
    film = O.film_vectors(P, P_, temb) if request.param else None
    return P, runs, (lambda which: (film[2 * which - 2], film[2 * which - 1])) if film else None


def _is_rel(line):
    """A rel-L2 line of Check.rel (not a float64 line, not a statistics line)."""
    return re.search(r" rel \d", line) is not None and "torch fp32" not in line


class _IO:
    """forced.LaunchIO over recorded states: `scale` multiplies what the launch wrote."""

    def __init__(self, before, after, out, scale):
        self._before, self._after, self._out, self.scale = before, after, out, scale

    def before(self, name):
        return self._before[name]

    def after(self, name):
        return self._after[name] * self.scale

    def out(self):
        return self._out * self.scale


def _feed(leaves, x, taps, H, strips):
    """[(before, after, out)] per launch: the level-0 buffers as the launches of this form leave them."""
    q, rows = forced.q, forced.rows
    g, S = taps["conv2_gate_pool"], taps["sca"]
    pooled = g.mean(dim=(2, 3)).reshape(-1)
    dev, feed = {"X0": rows(x)}, []
    for j, leaf in enumerate(leaves):
        before, prev = dict(dev), leaves[j - 1] if j else ""
        if leaf == "conv1":
            out = dev["T1_0"] = rows(taps["conv1"])
        elif leaf == "conv2_gate_pool":
            out = dev["G0"] = rows(q(g))
            if prev != "conv1" and not strips:
                dev["pooled0"], dev["pooled16_0"] = pooled, q(pooled)
        elif leaf == "pool_finish":
            out = dev["pooled0"] = pooled
        elif leaf == "sca":
            out = dev["S0"] = S.reshape(-1)
            if prev != "pool_finish" and H * H <= 16:
                dev["G0"] = rows(q(q(g) * S))
        elif leaf == "conv3":
            out = dev["Y0"] = rows(taps["conv3"])
            dev["Yb0"], dev["sy0"] = q(out), _partials(out.reshape(-1, C))
        elif leaf == "conv4":
            out = dev["G0"] = rows(q(taps["conv4"]))
        else:
            out = dev["X0"] = rows(taps["conv5"])
            dev["Xb0"], dev["sx0"] = q(out), _partials(out.reshape(-1, C))
            if strips:
                dev["pooled0"] = pooled
        feed.append((before, dict(dev), out))
    return feed


def _scan(block, H, leaves, extras, own_t1, strips, scale):
    P, runs, affine = block
    x, taps = runs[H]
    report = []
    ck = forced.Check(report)
    naf = forced.NafRules(P, ck, extras=extras, own_t1=own_t1)
    names = [f"{P_}.{leaf}" for leaf in leaves]
    for i, (before, after, out) in enumerate(_feed(leaves, x, taps, H, strips)):
        naf.launch(i, names, P_, 0, B, C, H, affine, _IO(before, after, out, scale))
    return report, ck


CASES = [("fused", FUSED, False), ("unfused", UNFUSED, False), ("chain", CHAIN, False), ("chain by strips", CHAIN, True), ("chain unfused", CHAIN_UNFUSED, False)]


@pytest.mark.parametrize("extras,own_t1", [(True, True), (False, False)], ids=["cr-prologue", "denoiser"])
@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rules_restate_the_oracle(block, monkeypatch, case, H, extras, own_t1):
    _, leaves, strips = case
    if strips:
        monkeypatch.setattr(forced, "STRIP_SHAPES", ((C, H),))
    report, ck = _scan(block, H, leaves, extras, own_t1, strips, 1.0)
    text = "\n".join(report)
    assert "no rule" not in text and "<<<<<<" not in text, text
    rel_lines = [ln for ln in report if _is_rel(ln)]
    # one line per output a form has: G (+ pooled), S (+ G*s), Y, G2, X, the chain's pooled; with extras the contributions
    t1 = own_t1 * (6 if H >= 8 else 5)                          # T1 and the band lines (a 4-row face has no band bottom)
    want = {"fused": 6 + (H == 4), "unfused": 6 + t1, "chain": 3, "chain by strips": 3, "chain unfused": 3 + t1}[case[0]]
    want += extras * (1 if "conv3" not in leaves else 2)
    assert len(rel_lines) == want, text
    for ln in rel_lines:
        assert float(re.search(r" rel (\S+) ", ln).group(1)) == 0.0, ln
    for ln in report:
        if "bit-exact" in ln:
            assert re.search(r" 0 of \d+ elements differ", ln), ln
    assert sum("bit-exact" in ln for ln in report) == extras * (("conv3" in leaves) + 1 + (leaves is FUSED or (leaves is CHAIN and not strips))), text
    assert ck.worst.get("stats", 0.0) <= forced.STAT_BOUND and ("stats" in ck.worst) == extras
    if own_t1 and "pool_finish" in leaves:
        err, err32 = ck.f64["pool_finish"]
        assert err <= forced.F64_MARGIN * err32 and ck.worst["pool_finish"] <= forced.FP32_BOUND, (err, err32)
    # the forms the launch names and the shape select
    sca = {"sca.prescale", "sca.scale_G"} if H == 4 else {"sca.bf16"}
    kinds = {"fused": {"conv2_gate_pool.fused", "conv3", "conv4", "conv5"} | sca,
             "unfused": {"conv2_gate_pool.unfused", "pool_finish", "sca.f32", "conv3", "conv4", "conv5"} | ({"conv1"} if own_t1 else set()),
             "chain": {"conv2_gate_pool.fused", "conv5.chain"}, "chain by strips": {"conv2_gate_pool.strips", "conv5.chain"},
             "chain unfused": {"conv2_gate_pool.unfused", "pool_finish", "conv5.chain"} | ({"conv1"} if own_t1 else set())}[case[0]]
    assert set(ck.worst) - {"stats", "bf16_copy"} == kinds, ck.worst


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_one_percent_error_flags_every_rel_line(block, monkeypatch, case):
    _, leaves, strips = case
    H = 4 if leaves is FUSED else 8
    if strips:
        monkeypatch.setattr(forced, "STRIP_SHAPES", ((C, H),))
    report, _ = _scan(block, H, leaves, True, True, strips, 1.01)
    rel_lines = [ln for ln in report if _is_rel(ln)]
    assert rel_lines and all(ln.endswith("<<<<<<") for ln in rel_lines), "\n".join(report)
