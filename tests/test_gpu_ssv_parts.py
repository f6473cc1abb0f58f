"""GPU tests of the long-target SSV scan in chained parts: nhmmer models of more nodes than one launch of the scan kernel
holds (6,142 .. 12,288), and the same chain forced onto small models (option ssv_parts), where a cut can go wrong at the
smallest size.  The device's window seeds against the oracle's sequential p7_SSVFilter_longtarget, both strands, every
flavour of the kernel; hmmer.nhmmer end to end against the CPU harness."""
import numpy as np
import pytest

import host_pipeline
from conftest import load_hmms, random_hmm
from pyhmmer_amd import _lib, easel, hmmer, plan7
from test_gpu_longtarget import SSV_KERNELS, device_seeds, rows_agree
from test_host_longtarget import _read, _rows
from test_host_ssv_parts import ssv_plan

pytestmark = pytest.mark.gpu


@pytest.fixture
def seams():
    """Sets the scan's options through the test seam; the library's own choices again afterwards."""
    yield lambda name, value: _lib.set_debug_option(name, value)
    _lib.set_debug_option("ssv_parts", 0)
    _lib.set_debug_option("ssv_kernel", -1)


def planted(hmm, L, stretches, seed, n_run=None):
    """<L> i.i.d. ACGT with the model's consensus of <n> nodes from node <first> at <pos>, a tenth of it mutated, for every
    (pos, first node, n) of <stretches>, on alternating strands; n_run: a run of N there."""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 4, size=L).astype(np.uint8)
    cons = np.argmax(hmm.match_emissions[1:], axis=1).astype(np.uint8)
    for c, (pos, first, n) in enumerate(stretches):
        seg = cons[first - 1:first - 1 + n].copy()
        mut = rng.random(len(seg)) < 0.1
        seg[mut] = rng.integers(0, 4, size=int(mut.sum()))
        seq[pos:pos + len(seg)] = seg if c % 2 == 0 else host_pipeline.DNA_COMP[seg[::-1]]
    if n_run is not None:
        seq[n_run:n_run + 30] = 15
    return seq


def seeds_equal_the_oracle(oracle, hmm, seq, seams, parts):
    """device_seeds == oracle.ssv_longtarget as lists, both strands, every entry of SSV_KERNELS, for every forced number of
    parts of <parts> (0: the library's plan).  The oracle's seeds per strand."""
    pli = plan7.LongTargetsPipeline(hmm.alphabet, block_length=1 << 30)
    om = plan7.OptimizedProfile(hmm, pli.background, 400)
    op = oracle.OracleProfile(hmm, pli.background, 400)
    wants = []
    for strand in (0, 1):
        blk = seq if strand == 0 else host_pipeline.DNA_COMP[seq[::-1]]
        want = oracle.ssv_longtarget(op, blk, hmm.max_length, pli.F1)
        for n in parts:
            seams("ssv_parts", n)
            for what, variant in SSV_KERNELS.items():
                seams("ssv_kernel", variant)
                got = device_seeds(om, pli._cfg(), seq, strand)
                assert got.tolist() == want.tolist(), (hmm.M, strand, n, what)
        wants.append(want)
    return wants


@pytest.mark.parametrize("M", [60, 250, 1000])
def test_forced_parts_on_small_models(M, oracle, seams):
    """2, 3 and 4 chained parts of models that one launch holds many times over: 100 kb of random sequence with 20 planted
    stretches of the consensus (any stretch longer than a part crosses a cut) and a run of N (the degenerate-residue path of
    every part)."""
    abc = easel.Alphabet.dna()
    hmm = random_hmm(M, seed=9000 + M, alphabet=abc)
    rng = np.random.default_rng(M)
    L = 100_000
    stretches = []
    for c in range(20):
        a = int(rng.integers(0, max(1, M - 40)))
        n = min(int(rng.integers(30, 400)), M - a)
        stretches.append((int(rng.integers(0, L - n)), a + 1, n))
    seq = planted(hmm, L, stretches, seed=M + 1, n_run=5000)
    parts = [n for n in (2, 3, 4) if M >= 2 * n]
    for n in parts:
        assert len(ssv_plan(M, 1, n)) == n and len(ssv_plan(M, 0, n)) == n
    wants = seeds_equal_the_oracle(oracle, hmm, seq, seams, parts)
    assert sum(len(w) for w in wants) >= 10


@pytest.mark.parametrize("nparts", [2, 3])
def test_forced_parts_bmyd(nparts, oracle, seams):
    """The fixture model (M = 1203; the every-second-row flavour is the library's choice for it) on its fixture target."""
    hmm = load_hmms("bmyD")[0]
    seq = np.asarray(_read("BGC0001090.gbk", hmm.alphabet)[0].sequence, dtype=np.uint8)
    assert len(ssv_plan(hmm.M, 1, nparts)) == nparts
    wants = seeds_equal_the_oracle(oracle, hmm, seq, seams, [nparts])
    assert sum(len(w) for w in wants) > 0


def test_forced_parts_across_separators(seams):
    """Three targets laid end to end are one scan with two one-residue separators, which floor every cell of every part and
    so the cut nodes' cells that go from part to part: the hits of the scan in 2, 3 and 4 parts are those of one launch."""
    hmm = load_hmms("bmyD")[0]
    abc = hmm.alphabet
    seq = np.asarray(_read("BGC0001090.gbk", abc)[0].sequence, dtype=np.uint8)
    cuts = [0, 15_000, 30_000, len(seq)]
    block = easel.DigitalSequenceBlock(abc, [easel.DigitalSequence(abc, name=f"part{q}", sequence=seq[a:b].copy()) for q, (a, b) in enumerate(zip(cuts, cuts[1:]))])
    one = _rows(next(hmmer.nhmmer(hmm, block, host_envelopes=1)))
    assert len(one) >= 1
    for n in (2, 3, 4):
        seams("ssv_parts", n)
        assert _rows(next(hmmer.nhmmer(hmm, block, host_envelopes=1))) == one, n


@pytest.mark.parametrize("M", [6141, 6142, 12288])
def test_models_beyond_one_launch(M, oracle, seams):
    """M = 6,142 and 12,288 in the library's own parts (6,141: the last model of one launch, unchanged), 250 kb with planted
    300-residue stretches of the consensus from node 1, from node M - 299, and around every cut node K of the plan from nodes
    K - 150 and K - 20, one of them laid across the first chunk boundary of the device scan.  The oracle's own list must hold a
    seed whose diagonal crosses every cut."""
    abc = easel.Alphabet.dna()
    hmm = random_hmm(M, seed=9000 + M, alphabet=abc)
    plans = [ssv_plan(M, pair) for pair in (0, 1)]
    cuts = sorted({hi for plan in plans for (_, hi, _) in plan[:-1]})
    assert (len(plans[1]) == 1) == (M == 6141) and (M < 12288 or len(cuts) >= 2)
    L = 250_000
    firsts = [1, M - 299] + [K - d for K in cuts for d in (150, 20)]
    chunk = ((8 * M + 63) // 64) * 64                                  # rows per chunk of the device scan for a target this short
    assert chunk + 1000 < L
    # one more, across the first chunk boundary (rows chunk / chunk + 1 of the forward strand): around the first cut, if there is one
    stretches = [(chunk - 150, firsts[2] if cuts else 1, 300)] + [(20_000 + 9_000 * c, f, 300) for c, f in enumerate(firsts)]
    assert all(p + 300 < chunk - 150 for p, _, _ in stretches[1:])
    seq = planted(hmm, L, stretches, seed=M, n_run=5000)
    wants = seeds_equal_the_oracle(oracle, hmm, seq, seams, [0])
    seeds = [s for w in wants for s in w.tolist()]                     # (first residue, last node, length of the diagonal)
    assert len(seeds) >= 10, len(seeds)
    for K in cuts:
        assert any(k - n + 1 <= K and K + 1 <= k for (_, k, n) in seeds), (K, sorted((k - n + 1, k) for (_, k, n) in seeds))


E2E = {}


def e2e_case(oracle, M):
    """The target, the model and the CPU harness' rows of an end-to-end case, computed once."""
    if M not in E2E:
        abc = easel.Alphabet.dna()
        hmm = random_hmm(M, seed=9000 + M, alphabet=abc)
        K = ssv_plan(M, 1)[0][1]
        seq = planted(hmm, 120_000, [(10_000, 1, 300), (40_000, K - 150, 300), (70_000, M - 299, 300), (100_000, M // 3, 300)], seed=M + 7)
        block = easel.DigitalSequenceBlock(abc, [easel.DigitalSequence(abc, name="target", sequence=seq)])
        ref = host_pipeline.host_nhmmer(oracle, hmm, block, pipeline=plan7.LongTargetsPipeline(abc, window_length=1200))
        E2E[M] = (hmm, block, _rows(ref), sum(1 for h in ref if h.reported))
    return E2E[M]


@pytest.mark.parametrize("where", [1, 2])
@pytest.mark.parametrize("M", [6200, 12288])
def test_nhmmer_end_to_end(M, where, oracle):
    """hmmer.nhmmer == the CPU harness (oracle scan + host tail) for models of 6,200 and 12,288 nodes: four planted hits, the
    envelopes rescored by the host workers (1) and by the envelope kernel's long-target instantiation (2)."""
    hmm, block, ref, nreported = e2e_case(oracle, M)
    assert nreported == 4
    rows_agree(_rows(next(hmmer.nhmmer(hmm, block, window_length=1200, host_envelopes=where))), ref)


def test_nhmmer_dealt_over_devices_in_parts(oracle):
    """The chunk_list path through the parts: the units of a search with a 6,200-node model dealt over two parts of one device."""
    hmm, block, ref, nreported = e2e_case(oracle, 6200)
    assert nreported == 4
    one = _rows(next(hmmer.nhmmer(hmm, block, window_length=1200, host_envelopes=1)))
    rows_agree(one, ref)
    assert _rows(next(hmmer.nhmmer(hmm, block, window_length=1200, devices=[0, 0], host_envelopes=1))) == one
