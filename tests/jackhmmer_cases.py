"""Shared by the jackhmmer tests: the queries and recorded rounds of the reference's own two runs, and the loop of
`plan7.IterativeSearch` with its two device steps replaced by their CPU seams.

The recorded rounds are tests/golden/msa/p12748-{1..3}.sto (`jackhmmer` of HMMER 3.3.2 with P12748 of LuxC.faa against the
fixture proteome) and KR-{1..6}.sto (KR.hmm against the proteome, "manually iterated hmmsearches" in the reference's words,
test_pipeline.py:301-328); of a file with two Stockholm records the first is the round's alignment."""
import numpy as np

import host_pipeline
from conftest import GOLDEN
from pyhmmer_amd import _lib, easel, plan7
from test_host_builder import fit, oracle_scores, stream_of

INC = 0.001             # jackhmmer's inclusion thresholds: Pipeline(incE=INC, incdomE=INC)
P12748_ROUNDS, KR_ROUNDS = 3, 6


def luxc_queries():
    with easel.SequenceFile(GOLDEN / "seqs" / "LuxC.faa", digital=True, alphabet=easel.Alphabet.amino()) as sf:
        return list(sf)


def p12748():
    return next(s for s in luxc_queries() if "P12748" in s.name)


def recorded(stem: str, n: int):
    """Round n of a recorded run: (columns, rows, alignment name, row names in order)."""
    with easel.MSAFile(GOLDEN / "msa" / f"{stem}-{n}.sto", digital=True, alphabet=easel.Alphabet.amino()) as f:
        msa = f.read()
    return len(msa), len(msa.names), msa.name, list(msa.names)


def shape_of(msa):
    return len(msa), len(msa.names), msa.name, list(msa.names)


def assert_codes_kept(msa):
    """The alignment of a round came with its code matrix, and the matrix is the text rows encoded."""
    assert getattr(msa, "_code_matrix", None) is not None
    assert msa._codes() is msa._code_matrix[0]
    assert np.array_equal(msa._codes(), msa._encode_rows())


class HostIterativeSearch(plan7.IterativeSearch):
    """`IterativeSearch` without a device: the search is the oracle's cascade followed by the product's host stage
    (host_pipeline.host_search), the model of a sequence or an alignment is the builder's host code (`_model`, `_model_msa`
    under the seam host_build = 1) calibrated as test_host_builder.py calibrates: the oracle's scores over
    p7x_calibration_stream, through p7x_calibration_fit."""

    def __init__(self, oracle, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.oracle = oracle

    def _search_hmm(self, hmm):
        return host_pipeline.host_search(self.oracle, hmm, self.targets, pipeline=self.pipeline)

    def _build(self, source):
        if isinstance(source, easel.DigitalMSA):
            _lib.set_debug_option("host_build", 1)
            try:
                hmm = self.builder._model_msa(source, self.background)
            finally:
                _lib.set_debug_option("host_build", -1)
        else:
            hmm = self.builder._model(source, self.background)
        op = self.oracle.OracleProfile(hmm, self.background, 100)
        om = plan7.OptimizedProfile(hmm, self.background, 100)
        sc, ovf, _ = oracle_scores(op, stream_of(self.background, seed=self.builder._calibration_seed()))
        st, ev = fit(sc, ovf, _lib.lib().p7x_oprofile_match_relent(om._handle))
        assert st == 0, _lib.last_error()
        hmm._evparam[:] = ev
        return hmm


def host_iterate(oracle, query, targets, select_hits=None, **pipeline_options):
    """What `Pipeline.iterate_seq` / `iterate_hmm` return, with the host steps in place of the device's."""
    pipeline = plan7.Pipeline(targets.alphabet, **{"incE": INC, "incdomE": INC, **pipeline_options})
    made = pipeline.iterate_hmm(query, targets, None, select_hits) if isinstance(query, plan7.HMM) else \
        pipeline.iterate_seq(query, targets, None, select_hits)
    return HostIterativeSearch(oracle, made.pipeline, made.builder, made.query, made.targets, made.select_hits)
