"""numpy restatements of ModelMixture::optimizeWeights (model/modelmixture.cpp:1355-1416, the EM of Wang, Li, Susko and Roger
2008 on the per-class pattern likelihoods of one tree evaluation) and of PhyloTree::computePatternStateFreq
(phylotree.cpp:1162-1196).  The matrix is rescaled in place by new_prop / prop after every step, as the reference does it."""
import numpy as np


def optimize_weights(lh_cat, ptn_freq, ptn_invar, prop, nsites=None, p_invar=None, max_steps=None):
    """lh_cat[nptn, nmix]: per-class pattern likelihoods (not modified), prop[nmix]: the class weights inside them.
    p_invar None or 0: no +I handling (the documented deviation: the reference would store the rounding noise of 1 - sum prop);
    otherwise ptn_invar belongs to p_invar and follows it linearly (computePtnInvar).
    -> dict(prop, p_invar, steps, converged, trace[steps, nmix + 1], last_change[steps]: max |prop - new_prop| per step)"""
    lk = np.array(lh_cat, dtype=np.float64)
    nptn, nmix = lk.shape
    freq = np.asarray(ptn_freq, dtype=np.float64)
    invar0 = np.zeros(nptn) if ptn_invar is None else np.asarray(ptn_invar, dtype=np.float64)
    invar = invar0.copy()
    prop = np.array(prop, dtype=np.float64)
    nsites = float(freq.sum()) if nsites is None else float(nsites)
    use_inv = p_invar is not None and p_invar > 0.0
    pinv0 = pinv = float(p_invar) if use_inv else 0.0
    max_steps = nmix if max_steps is None else max_steps
    ratio = np.ones(nmix)
    trace, change = [], []
    converged = False
    live = freq > 0.0
    for step in range(max_steps):
        if step > 0:
            lk *= ratio[None, :]
        new_prop = np.zeros(nmix)
        lk_ptn = invar.copy()
        for c in range(nmix):
            lk_ptn = lk_ptn + lk[:, c]
        t = np.zeros(nptn)
        t[live] = freq[live] / lk_ptn[live]
        for c in range(nmix):
            new_prop[c] = np.sum(lk[:, c] * t)
        new_prop /= nsites
        converged = bool(np.all(np.abs(prop - new_prop) < 1e-4))
        delta = float(np.max(np.abs(prop - new_prop)))
        ratio = new_prop / prop
        prop = new_prop.copy()
        new_pinvar = 0.0
        for c in range(nmix):
            new_pinvar += prop[c]
        new_pinvar = 1.0 - new_pinvar
        if use_inv:
            converged = converged and abs(pinv - new_pinvar) < 1e-4
            delta = max(delta, abs(pinv - new_pinvar))
            pinv = new_pinvar
            invar = invar0 * (pinv / pinv0)
        trace.append(np.concatenate([prop, [pinv]]))
        change.append(delta)
        if converged:
            break
    return dict(prop=prop, p_invar=pinv if use_inv else None, steps=len(trace), converged=int(converged),
                trace=np.array(trace), last_change=np.array(change))


def em_objective(lh_cat, ptn_freq, ptn_invar, scale):
    """sum_p freq_p log(ptn_invar_p + sum_m scale_m L_pm): the log-likelihood up to the patterns' scaling constants"""
    lk = np.asarray(lh_cat) * np.asarray(scale)[None, :]
    inv = 0.0 if ptn_invar is None else np.asarray(ptn_invar)
    return float(np.dot(ptn_freq, np.log(inv + lk.sum(axis=1))))


def posteriors(lh_cat):
    """phylotree.cpp:1174-1182: lh_cat[m] * (1 / sum_m lh_cat[m]), no invariant term"""
    lk = np.asarray(lh_cat, dtype=np.float64)
    s = np.zeros(lk.shape[0])
    for m in range(lk.shape[1]):
        s = s + lk[:, m]
    return lk * (1.0 / s)[:, None]


def pattern_state_freq(lh_cat, class_freq):
    """computePatternStateFreq: freq[p, state] = sum_m class_freq[m, state] post[p, m] (ascending m)"""
    post = posteriors(lh_cat)
    cf = np.asarray(class_freq, dtype=np.float64)
    out = np.zeros((post.shape[0], cf.shape[1]))
    for m in range(cf.shape[0]):
        out = out + post[:, m:m + 1] * cf[m][None, :]
    return out
