"""Models beyond 8,192 nodes without a device: the limit as a number, the profile tables, hmmpress and HMM.write round trips
of a model of 8,193 nodes, and the product's host stage against the oracle's domains on the fragment block of
tests/long_models.py -- the host side that tests/test_gpu_long_models.py compares the device with."""
import io

import numpy as np
import pytest

import host_pipeline
import long_models
from conftest import ROOT
from pyhmmer_amd import _lib, easel, hmmer, plan7
from test_oracle_domains import TOL_BITS

M = long_models.OLD_LIMIT + 1


def test_the_limit_is_a_number(libp7x):
    limit = libp7x.p7x_max_model_length()
    assert limit >= M and limit % 64 == 0
    assert long_models.long_lengths()[0] == M and long_models.long_lengths()[-1] == limit
    # the widest tier of the one list every dispatch expands
    header = (ROOT / "pyhmmer_amd" / "csrc" / "p7x_kernels.hpp").read_text()
    tiers = next(l for l in header.splitlines() if l.startswith("#define P7X_NODE_TIERS"))
    assert limit == 64 * int(tiers.rstrip().rsplit("X(", 1)[1].rstrip(")"))
    assert f"p7x_max_model_length" in (ROOT / "INTEGRATION.md").read_text()


def test_no_message_states_the_old_limit():
    for path in (ROOT / "pyhmmer_amd" / "csrc").glob("p7x_*"):
        for no, line in enumerate(path.read_text().splitlines(), 1):
            assert not ("too long" in line and "8192" in line), (path.name, no)


def test_profile_tables_of_a_model_beyond_the_old_limit(libp7x):
    hmm, bg, res, node, frags = long_models.case(M)
    om = plan7.OptimizedProfile(hmm, bg, 400)
    Q4, Q8, Q16 = (max(2, (M - 1) // w + 1) for w in (4, 8, 16))
    Kp = hmm.alphabet.Kp
    assert om.M == M and om.rbv.shape == (Kp, 16 * Q16) and om.rwv.shape == (Kp, 8 * Q8) and om.rfv.shape == (Kp, 4 * Q4)
    # the match odds, de-striped: node k = z Q + q + 1 sits at [q * 4 + z]
    k = np.arange(1, M + 1)
    pos = ((k - 1) % Q4) * 4 + (k - 1) // Q4
    f = bg.residue_frequencies.astype(np.float64)
    want = np.asarray(hmm.match_emissions, dtype=np.float64)[1:, :hmm.alphabet.K] / f[None, :hmm.alphabet.K]
    got = om.rfv[:hmm.alphabet.K][:, pos].T.astype(np.float64)
    assert np.allclose(got, want, rtol=2e-6, atol=1e-30)
    # the Viterbi filter's 16-bit scores of the same nodes: round(500 / ln 2 * ln odds), one unit for the float logarithm
    pos8 = ((k - 1) % Q8) * 8 + (k - 1) // Q8
    words = om.rwv[:hmm.alphabet.K][:, pos8].T.astype(np.float64)
    assert np.abs(words - np.maximum(np.round(500.0 / np.log(2.0) * np.log(want)), -32768.0)).max() <= 1.0


def test_hmmpress_and_hmm_write_round_trips(libp7x, tmp_path):
    hmm, bg, res, node, frags = long_models.case(M)
    assert hmmer.hmmpress([hmm], tmp_path / "long") == 1
    ref = plan7.OptimizedProfile(hmm, bg, 400)
    with plan7.HMMPressedFile(tmp_path / "long") as pressed:
        assert len(pressed) == 1
        om = next(iter(pressed))
        assert (om.name, om.M, om.consensus) == (hmm.name, M, hmm.consensus)
        assert (om.tbm, om.tec, om.tjb, om.base, om.bias) == (ref.tbm, ref.tec, ref.tjb, ref.base, ref.bias)
        for tab in ("rbv", "sbv", "rwv", "twv", "rfv", "tfv"):
            a, b = getattr(om, tab), getattr(ref, tab)
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), tab
    for binary in (False, True):
        buf = io.BytesIO()
        hmm.write(buf, binary=binary)
        buf.seek(0)
        back = list(plan7.HMMFile(buf))
        assert len(back) == 1 and back[0].M == M and back[0].name == hmm.name and back[0].consensus == hmm.consensus
        if binary:
            assert np.array_equal(back[0].match_emissions, hmm.match_emissions)
            assert np.array_equal(back[0].transition_probabilities, hmm.transition_probabilities)
        else:           # the text form prints five decimals of -ln p
            assert np.allclose(back[0].match_emissions, hmm.match_emissions, rtol=2e-5, atol=1e-7)
            assert np.allclose(back[0].transition_probabilities, hmm.transition_probabilities, rtol=2e-5, atol=1e-7)
        again = plan7.OptimizedProfile(back[0], bg, 400)
        if binary:
            assert np.array_equal(again.rfv.view(np.uint8), ref.rfv.view(np.uint8))


def test_host_stage_agrees_with_the_oracle_on_the_fragment_block(oracle):
    """The host stage (what the GPU tests compare the device with) against the oracle's domains, both fed the oracle's parser
    rows: every fragment is one domain with the oracle's envelope, alignment and model coordinates and its scores to
    TOL_BITS; of the three two-copy targets at least one is one region that a traceback ensemble resolves."""
    hmm, bg, res, node, frags = long_models.case(M)
    block = long_models.domain_block(M)
    pli = plan7.Pipeline(hmm.alphabet, E=1e3, domE=1e3)
    hits = host_pipeline.host_search(oracle, hmm, block, pipeline=pli)
    by_hit = {h.name: h for h in hits}
    assert all(f"frag{i}" in by_hit for i in range(6)) and all(f"two{i}" in by_hit for i in range(3))
    op = oracle.OracleProfile(hmm, pli.background, 400)
    by_name = {s.name: s for s in block}
    C = long_models.nodes_per_lane(M)
    crossing = 0
    for i in range(6):
        h = by_hit[f"frag{i}"]
        envs, counts = oracle.domains_single(op, np.asarray(by_name[h.name].sequence, dtype=np.uint8))
        assert h.nregions == counts[0] and len(envs) >= 1
        prod = {(d.env_from, d.env_to): d for d in h.domains}
        for e in envs:
            d = prod.get((int(e[0]), int(e[1])))
            assert d is not None, (h.name, e[:2], sorted(prod))
            a = d.alignment
            assert (a.target_from, a.target_to, a.hmm_from, a.hmm_to) == tuple(int(v) for v in e[2:6]), h.name
            assert abs(d.score - e[9]) <= TOL_BITS and abs(d.bias - e[10]) <= TOL_BITS, (h.name, d.score, e[9], d.bias, e[10])
            crossing += (a.hmm_from - 1) // C != (a.hmm_to - 1) // C
    assert crossing >= 3                      # alignments that run across a boundary between two lanes of the 192-node layout
    lo, hi = zip(*[(d.alignment.hmm_from, d.alignment.hmm_to) for i in range(6) for d in by_hit[f"frag{i}"].domains])
    assert min(lo) <= 5 and max(hi) >= M - 5  # ... the first lane and the last
    twos = [by_hit[f"two{i}"] for i in range(3)]
    assert all(len(h.domains) == 2 for h in twos)
    assert any(h.nregions == 1 and h.nclustered == 1 for h in twos), [(h.nregions, h.nclustered) for h in twos]


GRANTED_SCRATCH = 13488      # bytes per lane: env_kernel<192>, the largest request of the envelope unit that the MI355X runtime granted
                             # both in a process of its own and in the process that runs the whole GPU suite


def test_no_envelope_instantiation_asks_for_more_scratch_than_was_seen_granted(libp7x, tmp_path):
    """env_kernel<576> (40,368 bytes of scratch per lane) and, late in a long process, env_kernel<320> (22,448) had their queue
    aborted by the runtime: a tier added to P7X_NODE_TIERS must keep every instantiation of the envelope unit --
    the hungriest -- within what was granted in both settings."""
    import re
    import shutil
    import subprocess
    asm = _lib.fresh_isa("p7x_envelope.hip")             # what build() compiled, if it is current; else compile the unit here
    if asm is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        asm = tmp_path / "envelope.s"
        subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-S",
                        "--cuda-device-only", "-I", str(ROOT / "include"), "-o", str(asm), str(ROOT / "pyhmmer_amd/csrc/p7x_envelope.hip")],
                       check=True, capture_output=True)
    sizes = [int(v) for v in re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", asm.read_text(), re.M)]
    widest = libp7x.p7x_max_model_length() // 64
    assert len(sizes) >= 50 and max(sizes) >= 60 * widest, (len(sizes), max(sizes))        # the long tiers are among them (about 70 bytes per node)
    assert max(sizes) <= GRANTED_SCRATCH, max(sizes)
