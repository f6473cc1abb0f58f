"""Gap-rich synthetic models and the targets that make their D->D chains decide the Viterbi score (test input only).

conftest.random_hmm draws deletion-poor transitions (tMD <= 0.07, tDD <= 0.5) and test_gpu_filters._model_block emits
fragments that saturate the 16-bit score, so neither says much about the lazy-F closure of the Viterbi kernels: the
in-register D->D walk, the carry from one stripe (packed kernel) or lane (wave-per-target kernel) into the next, and the
repetition of both until nothing improves.  Here a model gets DELETION CORRIDORS, runs of nodes with tDD >= 0.95 that
are longer than three stripes of the kernel instantiation that runs the model, and a target is the consensus of a few
nodes before a corridor followed by the consensus of a few nodes after it: short enough not to saturate, and worth
more as one domain that deletes the corridor than as two.  tests/test_host_vit_gaps.py measures, with the numpy
restatement of the packed kernel, how many of these targets change their score when the closure is cut short."""
import numpy as np

from conftest import random_hmm

# columns of HMM.transition_probabilities
MM, MI, MD, IM, II, DM, DD = range(7)

_PK8 = (2, 4, 6, 8, 10, 12, 14, 15, 16, 17, 18, 19, 20)        # register pairs per lane of the packed kernel, T = 8 lanes
_PK16 = (11, 12, 13, 14, 15, 16, 17, 18, 19, 20)                # ... T = 16 lanes
_TIERS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 96, 128)      # nodes per lane of the wave-per-target kernels


def packed_shape(M):
    """(T, P) of the packed Viterbi kernel for a model of M nodes (p7x_vitpk.hip: vitpk_pick), None beyond 640 nodes."""
    for p in _PK8:
        if M <= 16 * p:
            return 8, p
    for p in _PK16:
        if M <= 32 * p:
            return 16, p
    return None


def wave_nodes_per_lane(M):
    """Nodes per lane C of the wave-per-target kernels (p7x_vitfwd.hip: vit_pick_C)."""
    need = (M + 63) // 64
    return next(c for c in _TIERS if c >= need)


def stripe_nodes(M):
    """Consecutive nodes that one stripe of the Viterbi filter holds: P where the packed kernel takes the model (its
    stripes are the longer ones when both kernels do, M <= 640), else the wave-per-target kernel's nodes per lane."""
    pk = packed_shape(M)
    return pk[1] if pk else wave_nodes_per_lane(M)


def gappy_hmm(M, seed, alphabet=None, conserved=0.8):
    """random_hmm (same boundary conventions, consensus, _evparam, max_length) with deletion corridors and insert-rich
    nodes.  The model is: ordinary stretch (9-12 nodes), corridor, ordinary stretch, corridor, ..., ordinary stretch.
      corridor        3P+1 .. 4P+1 nodes (P = stripe_nodes(M)): tDD in [0.95, 1) on all but the last, which is the way out
                      (tDM 0.6-0.8); tMD 0.3-0.45 on these nodes and on the node before the corridor, the way in.  Long
                      corridors get tDD nearer to one, so that deleting one costs about as much at every model length.
      insert-rich     the fourth node from the end of every other ordinary stretch: tMI 0.2-0.3, tII 0.9-0.95."""
    hmm = random_hmm(M, seed, alphabet, conserved)
    rng = np.random.default_rng([int(seed), int(M), 77])
    per = stripe_nodes(M)
    t = np.array(hmm.transition_probabilities, dtype=np.float64)
    k, n = 1, 0
    while True:
        o, Lc = int(rng.integers(9, 13)), 3 * per + 1 + int(rng.integers(0, per + 1))
        if k + o + Lc + 9 - 1 > M:
            break
        c0 = k + o                      # first node of the corridor; c0 - 1 is the way in
        c1 = c0 + Lc - 1                # the way out
        eps = min(0.05, 2.0 / Lc)
        t[c0:c1, DD] = 1.0 - rng.uniform(0.2, 1.0, size=Lc - 1) * eps
        t[c1, DD] = rng.uniform(0.2, 0.4)
        t[c0:c1 + 1, DM] = 1.0 - t[c0:c1 + 1, DD]
        t[c0 - 1:c1 + 1, MD] = rng.uniform(0.3, 0.45, size=Lc + 1)
        t[c0 - 1:c1 + 1, MI] = rng.uniform(0.01, 0.03, size=Lc + 1)
        if n % 2 == 0:
            r = c0 - 4
            t[r, MI], t[r, MD] = rng.uniform(0.2, 0.3), rng.uniform(0.006, 0.03)
            t[r, II] = rng.uniform(0.9, 0.95)
            t[r, IM] = 1.0 - t[r, II]
        t[c0 - 4:c1 + 1, MM] = 1.0 - t[c0 - 4:c1 + 1, MI] - t[c0 - 4:c1 + 1, MD]
        k, n = c1 + 1, n + 1
    assert n >= 1, f"no room for a deletion corridor in {M} nodes"
    hmm.transition_probabilities[:] = t
    return hmm


def corridors(hmm):
    """[(c0, c1)]: the D states c0 .. c1 are cheap to walk through; c0 - 1 is the way in, c1 + 1 the first node after."""
    dd = np.asarray(hmm.transition_probabilities, dtype=np.float64)[:, DD] >= 0.9499
    out, k = [], 1
    while k <= hmm.M:
        if dd[k]:
            c0 = k
            while dd[k]:
                k += 1
            out.append((c0, k))
        k += 1
    return out


def insert_rich(hmm):
    t = np.asarray(hmm.transition_probabilities, dtype=np.float64)
    return [int(k) for k in np.nonzero((t[:, MI] >= 0.199) & (t[:, II] >= 0.899))[0] if 1 <= k < hmm.M]


def _background(hmm):
    from pyhmmer_amd import plan7
    p = plan7.Background(hmm.alphabet).residue_frequencies.astype(np.float64)
    return p / p.sum()


def bridge_targets(hmm, n, seed):
    """n DigitalSequences: flank (0-12 background residues), the consensus of the 3-8 nodes before a corridor, the
    consensus of the 3-8 nodes after it, flank.  One target in five bridges two neighbouring corridors (3-5 nodes before
    the first, the whole stretch between them, 3-5 after the second); one in five has 5-30 background residues
    inserted at the insert-rich node three nodes before the corridor.  The matched stretches are short on purpose: the
    16-bit score must not saturate."""
    from pyhmmer_amd import easel
    abc = hmm.alphabet
    rng = np.random.default_rng([int(seed), int(hmm.M), 78])
    bgp = _background(hmm)
    cons = np.argmax(np.asarray(hmm.match_emissions), axis=1).astype(np.uint8)
    cors, rich = corridors(hmm), set(insert_rich(hmm))
    with_insert = [j for j, (c0, c1) in enumerate(cors) if c0 - 4 in rich]

    def noise(lo, hi):
        return rng.choice(abc.K, size=int(rng.integers(lo, hi + 1)), p=bgp).astype(np.uint8)

    out = []
    for i in range(n):
        kind = i % 5
        if kind == 3 and len(cors) >= 2:
            j = int(rng.integers(0, len(cors) - 1))
            (a0, a1), (b0, b1) = cors[j], cors[j + 1]
            a, b = int(rng.integers(3, 6)), int(rng.integers(3, 6))
            core = [cons[a0 - a:a0], cons[a1 + 1:b0], cons[b1 + 1:b1 + 1 + b]]
        elif kind == 4 and with_insert:
            c0, c1 = cors[with_insert[int(rng.integers(0, len(with_insert)))]]
            b = int(rng.integers(3, 9))
            core = [cons[c0 - 6:c0 - 3], noise(5, 30), cons[c0 - 3:c0], cons[c1 + 1:c1 + 1 + b]]
        else:
            c0, c1 = cors[int(rng.integers(0, len(cors)))]
            a, b = int(rng.integers(3, 9)), int(rng.integers(3, 9))
            core = [cons[c0 - a:c0], cons[c1 + 1:c1 + 1 + b]]
        seq = np.concatenate([noise(0, 12)] + core + [noise(0, 12)])
        out.append(easel.DigitalSequence(abc, name=f"bridge{i}", sequence=seq))
    return out


def with_background_neighbours(targets, seed):
    """Every target followed by an i.i.d. background sequence of the same length.  A SequenceDatabase sorts its targets by
    length before it forms wavefronts, so a target that asks for the D->D closure shares its wavefront with targets
    that do not: the packed kernel then walks their registers too and must keep the carry from them."""
    from pyhmmer_amd import easel, plan7
    abc = targets[0].alphabet
    p = plan7.Background(abc).residue_frequencies.astype(np.float64)
    p /= p.sum()
    rng = np.random.default_rng([int(seed), 79])
    out = []
    for i, s in enumerate(targets):
        out.append(s)
        out.append(easel.DigitalSequence(abc, name=f"neighbour{i}", sequence=rng.choice(abc.K, size=len(s), p=p).astype(np.uint8)))
    return out


def without_delete_chains(hmm):
    """A copy of the model whose D->D mass has been moved into D->M (tDD = 1e-6): a score that differs between the two
    comes from a path that deletes more than one node in a row."""
    from pyhmmer_amd import plan7
    cp = plan7.HMM(hmm.alphabet, hmm.M, hmm.name + "_nodd")
    t = np.array(hmm.transition_probabilities, dtype=np.float64)
    t[1:hmm.M, DD] = 1e-6
    t[1:hmm.M, DM] = 1.0 - 1e-6
    cp.transition_probabilities[:] = t
    cp.match_emissions[:] = hmm.match_emissions
    cp.insert_emissions[:] = hmm.insert_emissions
    cp.composition = np.array(hmm.composition, dtype=np.float32)
    cp.consensus = hmm.consensus
    cp._evparam[:] = hmm._evparam
    cp.max_length = hmm.max_length
    return cp
