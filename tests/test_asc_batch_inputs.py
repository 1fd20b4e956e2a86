"""CPU: every +ASC input of tests/test_asc_batch_gpu.py is a usable one -- the oracle alone gives a finite lnL with
prob_const in [0, 1) (OracleTree.branch_lnl asserts the range) and finite corrected derivatives on the root branch, so no
case of the GPU file can turn out degenerate on the card."""
import numpy as np
import pytest

import test_asc_batch_gpu as G

ALL = sorted(set(G.NNI1_CASES + G.NNI5_CASES + G.ORACLE_CASES + [G.ABI_CASE] + G.SHARD_CASES + G.SWEEP_CASES +
                 [G.SWEEP_DIVERGED_CASE]))


@pytest.mark.parametrize("n,ncat,seq_type,ntaxa,nsites", ALL)
def test_asc_inputs_are_usable(synth, oracle, n, ncat, seq_type, ntaxa, nsites):
    inputs = G.asc_inputs(synth, n, ncat, seq_type, ntaxa, nsites)
    nwk, pat, freq, nun, ns, model = inputs
    assert nun == n and ns == freq.sum() > 0 and pat.shape[1] > 2 * n
    assert not np.any(np.all(pat[:, :-nun] == pat[0][None, :-nun], axis=0))      # variable sites only
    ot = G.asc_oracle(oracle, inputs, n, seq_type)
    lnl, (a, b) = ot.likelihood()
    assert np.isfinite(lnl) and lnl < 0.0
    df, ddf = ot.derv(a, b)
    assert np.isfinite(df) and np.isfinite(ddf)
