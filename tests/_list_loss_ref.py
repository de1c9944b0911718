"""The list losses of include/cffm_hip.h (cffm_list_loss) read loop by loop in float64 - the formulae of the header and nothing else.

scores [G, Lg], target [G] positions.  With t = target[g] and m = Lg - 1:

  bpr       terms[g] = (1/m) sum_{n != t} softplus(s_n - s_t);  dout[g, n] = sigmoid(s_n - s_t) / (G m),  dout[g, t] = -sum_{n != t} dout[g, n]
  softmax   terms[g] = log sum_n exp(s_n - max) + max - s_t;    dout[g, n] = (p_n - [n = t]) / G
  loss = (1/G) sum_g terms[g]

A NaN score makes its list's term and whole dout row NaN (and the loss); a target outside [0, Lg) gives a zero term and a zero row.
The `fault` argument plants one of four mistakes, for the test that shows the criterion would catch them."""
import math

import numpy as np

KINDS = ('bpr', 'softmax')


def _softplus(x):
    return max(x, 0.0) + math.log1p(math.exp(-abs(x)))


def _sigmoid(x):
    e = math.exp(-abs(x))
    return 1.0 / (1.0 + e) if x >= 0 else e / (1.0 + e)


def list_loss_ref(kind, scores, target, fault=None):
    """-> (loss float, dout float64 [G, Lg], terms float64 [G])"""
    assert kind in KINDS and fault in (None, 'sign', 'normaliser', 'target0', 'no_max')
    s = np.asarray(scores, dtype=np.float64)
    G, Lg = s.shape
    m = Lg - 1
    dout, terms = np.zeros((G, Lg)), np.zeros(G)
    for g in range(G):
        t = 0 if fault == 'target0' else int(target[g])
        if t < 0 or t >= Lg:
            continue
        if np.isnan(s[g]).any():
            terms[g], dout[g] = np.nan, np.nan
            continue
        if kind == 'bpr':
            norm = G if fault == 'normaliser' else G * m
            acc, tot = 0.0, 0.0
            for n in range(Lg):
                if n == t:
                    continue
                x = s[g, n] - s[g, t]
                if fault == 'no_max':                    # log(1 + exp(x)) as float32 would form it: inf from x > 88.7
                    with np.errstate(over='ignore'):
                        acc += float(np.log(np.float32(1) + np.exp(np.float32(x))))
                else:
                    acc += _softplus(x)
                dout[g, n] = _sigmoid(x) / norm
                tot += dout[g, n]
            terms[g] = acc / m
            dout[g, t] = tot if fault == 'sign' else -tot
        else:
            mx = 0.0 if fault == 'no_max' else max(s[g])
            ft = np.float32 if fault == 'no_max' else np.float64     # exp(s_n) as float32 would form it: inf from s_n > 88.7
            with np.errstate(over='ignore', invalid='ignore'):
                e = [np.float64(np.exp(ft(s[g, n] - mx))) for n in range(Lg)]
                den = ft(sum(e))
                terms[g] = np.log(den) + mx - s[g, t]
                for n in range(Lg):
                    dout[g, n] = (e[n] / den - (1.0 if n == t else 0.0)) / G
            if fault == 'sign':
                dout[g, t] = -dout[g, t]
    return float(np.sum(terms) / G) if G else 0.0, dout, terms
