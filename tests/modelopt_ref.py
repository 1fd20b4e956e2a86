"""The model-parameter optimisers restated in Python on textbook likelihoods (tests/textbook.py: probability-space pruning,
scipy expm, no eigen-space vectors): ModelGTR::optimizeParameters over bfgs_ref, RateGamma / RateInvar / RateGammaInvar
optimizeParameters over em_ref's Brent, and the loop of ModelFactory::optimizeParameters with fixed branch lengths.  The
likelihood is cached per parameter vector; the trees and alignments of the tests are small enough for the CPU."""
import numpy as np

import bfgs_ref
import em_ref
import textbook

MIN_RATE, MAX_RATE, TOL_RATE = 1e-4, 100.0, 1e-4
MIN_GAMMA_SHAPE, MAX_GAMMA_SHAPE, TOL_GAMMA_SHAPE = 0.02, 1000.0, 0.001
MIN_PINVAR, TOL_PINVAR = 1e-6, 1e-6
GRADIENT_EPSILON = 0.0001
LOGL_EPSILON = 0.01


class Problem:
    """adj: the tree as textbook takes it; pat / freq: patterns and their frequencies; exch(params) -> the symmetric
    exchangeability matrix; state_freq fixed; ncat Gamma categories (1: none); has_invar; frac_const: the alignment's
    fraction of constant sites"""

    def __init__(self, synth, adj, pat, freq, seq_type, su, exch, state_freq, ncat, has_gamma, has_invar, frac_const):
        self.synth, self.adj, self.pat, self.freq = synth, adj, pat, np.asarray(freq, dtype=np.float64)
        self.seq_type, self.su, self.exch, self.state_freq = seq_type, su, exch, np.asarray(state_freq, dtype=np.float64)
        self.ncat, self.has_gamma, self.has_invar, self.frac_const = ncat, has_gamma, has_invar, frac_const
        n = len(self.state_freq)
        self.const = np.all(pat == pat[0:1], axis=0) & (pat[0] < n)
        self.const_freq = np.where(self.const, self.state_freq[np.minimum(pat[0], n - 1)], 0.0)
        self.cache = {}
        self.evaluations = 0

    def lnl(self, params, alpha, pinv):
        key = (tuple(float(p) for p in params), float(alpha), float(pinv))
        if key not in self.cache:
            self.evaluations += 1
            model = self.synth.reversible_model(self.exch(key[0]), self.state_freq, alpha if self.ncat > 1 else None, self.ncat, pinv)
            logs = textbook.site_log_likelihoods(self.adj, self.pat, model, self.seq_type, self.su)
            if pinv > 0.0:
                iv = pinv * self.const_freq
                logs = np.where(iv > 0.0, np.logaddexp(logs, np.log(np.where(iv > 0.0, iv, 1.0))), logs)
            self.cache[key] = float(np.dot(self.freq, logs))
        return self.cache[key]


def gtr_exch(params):
    a, b, c, d, e = params
    return np.array([[0, a, b, c], [a, 0, d, e], [b, d, 0, 1.0], [c, e, 1.0, 0]], dtype=np.float64)


def optimize_model(pb, params, alpha, pinv, gradient_epsilon=GRADIENT_EPSILON, gradients=None):
    """ModelGTR::optimizeParameters -> (params, lnl)"""
    n = len(params)
    if n == 0:
        return list(params), 0.0
    res = bfgs_ref.minimize_multi_dimen(lambda x: -pb.lnl(x, alpha, pinv), params, [MIN_RATE] * n, [MAX_RATE] * n, [False] * n,
                                        max(gradient_epsilon, TOL_RATE), gradients)
    return res["x"], pb.lnl(res["x"], alpha, pinv)


def optimize_rates(pb, params, alpha, pinv, gradient_epsilon=GRADIENT_EPSILON):
    """RateGammaInvar (alpha, then p-inv) / RateGamma / RateInvar::optimizeParameters -> (alpha, pinv, lnl)"""
    lh = 0.0
    if pb.has_gamma:
        alpha, _, _ = em_ref.minimize_one_dimen(lambda a: -pb.lnl(params, a, pinv), MIN_GAMMA_SHAPE, alpha, MAX_GAMMA_SHAPE,
                                                max(gradient_epsilon, TOL_GAMMA_SHAPE))
        lh = pb.lnl(params, alpha, pinv)
    if pb.has_invar:
        pinv, _, _ = em_ref.minimize_one_dimen(lambda p: -pb.lnl(params, alpha, p), MIN_PINVAR, pinv,
                                               min(pb.frac_const, 1.0 - MIN_PINVAR), max(gradient_epsilon, TOL_PINVAR))
        lh = pb.lnl(params, alpha, pinv)
    return alpha, pinv, lh


def optimize_parameters(pb, params, alpha, pinv, logl_epsilon=LOGL_EPSILON, gradient_epsilon=GRADIENT_EPSILON):
    """ModelFactory::optimizeParameters with fixed_len -> dict(params, alpha, pinv, lnl, rounds, trace of lnL)"""
    cur = pb.lnl(params, alpha, pinv)
    trace = [cur]
    i = 2
    for i in range(2, 100):
        params, model_lh = optimize_model(pb, params, alpha, pinv, gradient_epsilon)
        alpha, pinv, rate_lh = optimize_rates(pb, params, alpha, pinv, gradient_epsilon)
        new = model_lh if rate_lh == 0.0 else rate_lh
        trace.append(new)
        if new == 0.0:
            break
        if new > cur + logl_epsilon:
            cur = new
        else:
            break
    return dict(params=list(params), alpha=alpha, pinv=pinv, lnl=pb.lnl(params, alpha, pinv), rounds=i - 1, trace=trace)
