"""CPU: the EM restatement (tests/em_oracle.py) on the reference's saved EN model, and the EM optimizer's
host-side surface (the optimizer switch and Spark's parameter rules)."""
import os

import numpy as np
import pytest

import em_oracle as E
from helpers import GOLDEN

REF_MODEL = os.path.join(GOLDEN, "LdaModel_EN_1591049082850")


@pytest.fixture(scope="module")
def golden():
    import stc

    m = stc.io.load_distributed(REF_MODEL)
    src, term, cnt = E.edges_of_model(m)
    return m, src, term, cnt


def test_golden_model_mass_identities(golden):
    """each document's topic counts sum to its edge weights, each term's to its column weight, and
    globalTopicTotals = Σ_w N_wk (measured 1.2e-14, 9.3e-16, 3.8e-13)"""
    m, src, term, cnt = golden
    assert src.size == 253368 and m["doc_topics"].shape == (51, 5) and m["topics"].shape == (39380, 5)
    errs = E.mass_identities(m["doc_topics"], m["topics"], m["global_topic_totals"], src, term, cnt)
    assert max(errs) <= 1e-11, errs


def test_one_restated_step_preserves_the_mass_identities(golden):
    m, src, term, cnt = golden
    alpha, eta = float(m["alpha"][0]), m["eta"]
    ndk, nwk, nk = E.step(m["doc_topics"], m["topics"], m["global_topic_totals"], src, term, cnt, alpha, eta)
    assert np.all(ndk > 0) and np.all(nwk > 0)
    errs = E.mass_identities(ndk, nwk, nk, src, term, cnt)
    assert max(errs) <= 1e-11, errs


def test_golden_log_likelihood_anchor(golden):
    """regression anchor: the restatement's logLikelihood of the saved state"""
    m, src, term, cnt = golden
    ll = E.log_likelihood(m["doc_topics"], m["topics"], m["global_topic_totals"], src, term, cnt,
                          float(m["alpha"][0]), m["eta"])
    assert abs(ll - (-6374174.85)) <= 1e-9 * 6374174.85, ll


def test_optimizer_switch_accepts_em():
    import stc

    lda = stc.MllibLDA().setOptimizer("em")
    assert isinstance(lda.optimizer, stc.EMLDAOptimizer)
    opt = stc.EMLDAOptimizer().setKeepLastCheckpoint(False)
    assert opt.getKeepLastCheckpoint() is False
    assert stc.MllibLDA().setOptimizer(opt).optimizer is opt
    assert isinstance(stc.MllibLDA().setOptimizer("online").optimizer, stc.OnlineLDAOptimizer)
    with pytest.raises(ValueError):
        stc.MllibLDA().setOptimizer("gibbs")
    with pytest.raises(ValueError):
        stc.LDA(optimizer="em")  # the ml estimator is not where the reference selects EM


def test_em_parameter_rules():
    import stc

    assert stc.em_concentrations(5) == (11.0, 1.1)
    assert stc.em_concentrations(100, -1.0, -1.0) == (1.5, 1.1)
    assert stc.em_concentrations(3, [2.0, 2.0, 2.0], 1.5) == (2.0, 1.5)
    corpus = stc.CsrMatrix.from_rows([([0, 1], [1.0, 2.0]), ([1], [1.0])], 4)
    for alpha, eta in ((1.0, -1.0), (0.5, -1.0), (-1.0, 1.0), (-1.0, 0.1), ([2.0, 3.0, 2.0], -1.0)):
        lda = stc.MllibLDA().setOptimizer("em").setK(3).setDocConcentration(alpha).setTopicConcentration(eta)
        with pytest.raises(ValueError):
            lda.run(corpus)  # raises before any device is touched
