"""Float64 numpy restatement of the occupancy loss's scene-class affinity terms (gaussianformer_amd/occupancy_loss.py
docstring; the reference's sem_scal_loss / geo_scal_loss): per layer sem, geo and their gradient.

The sums S_c, N_c are float64 (the softmax too); each is rounded to fp32 once, and the tail -- every ratio, the shift loops
of inverse_sigmoid and f -- is fp32, operation by operation, because the contract says so: whether a ratio takes a shift step
depends on its fp32 value (a perfect specificity is exactly 1.0f and takes two).  The derivative is the analytic -1/x' in
float64 from the fp32 values.
"""
import numpy as np

import occ_loss_ref

F32 = np.float32
EPS = F32(1e-5)
HI = F32(1.0 - 1e-5)
MAX_STEPS = 8


def scal_f(x):
    """(f, f', ok) of an fp32 ratio x: the two shift loops (at most MAX_STEPS steps each), f = softplus(log(1/x - 1))."""
    x = F32(x)
    for _ in range(MAX_STEPS):
        if not x >= HI:
            break
        x = F32(x - EPS)
    for _ in range(MAX_STEPS):
        if not x < EPS:
            break
        x = F32(x + EPS)
    ok = bool(x >= EPS and x < HI)
    with np.errstate(all="ignore"):
        u = np.log(F32(F32(1) / x) - F32(1), dtype=F32)
        f = F32(max(u, F32(0)) + np.log1p(np.exp(-abs(u), dtype=F32), dtype=F32)) if np.isfinite(u) else F32(np.nan)
        d = -1.0 / float(x)
    return f, d, ok


def scal_terms(S64, N64, T, empty_label):
    """One layer: S64, N64 float64 [C] sums, T int [C].  Returns (sem, geo, a [C], b [C], ok) with a = d(sem, geo)/dS as two
    rows (sem, geo) -- unweighted -- and b likewise by N."""
    C = len(T)
    V = int(T.sum())
    S, N = S64.astype(F32), N64.astype(F32)
    a = np.zeros((2, C))
    b = np.zeros((2, C))
    ok = True
    classes = [i for i in range(C - 1) if T[i] > 0]
    count = len(classes)
    total = F32(0)
    for i in classes:
        cls = F32(0)
        Tf = F32(T[i])
        if S[i] > 0:
            den = F32(S[i] + EPS)
            x = F32(N[i] / den)
            f, d, k = scal_f(x)
            ok &= k
            cls = F32(cls + f)
            a[0, i] -= d * float(x) / float(den)
            b[0, i] += d / float(den)
        den = F32(Tf + EPS)
        f, d, k = scal_f(F32(N[i] / den))
        ok &= k
        cls = F32(cls + f)
        b[0, i] += d / float(den)
        if V - T[i] > 0:
            R = F32(V - T[i])
            den = F32(R + EPS)
            f, d, k = scal_f(F32(F32(R - F32(S[i] - N[i])) / den))
            ok &= k
            cls = F32(cls + f)
            a[0, i] -= d / float(den)
            b[0, i] += d / float(den)
        total = F32(total + cls)
    if count:
        sem = F32(total / F32(count))
        a[0] /= count
        b[0] /= count
    else:
        sem, ok = F32(np.nan), False
    e = empty_label
    R = F32(V - T[e])
    I = F32(R - F32(S[e] - N[e]))
    d1, d2, d3 = F32(F32(F32(V) - S[e]) + EPS), F32(R + EPS), F32(F32(T[e]) + EPS)
    x1, x2, x3 = F32(I / d1), F32(I / d2), F32(N[e] / d3)
    (f1, g1, k1), (f2, g2, k2), (f3, g3, k3) = scal_f(x1), scal_f(x2), scal_f(x3)
    ok &= k1 and k2 and k3
    geo = F32(F32(f1 + f2) + f3)
    a[1, e] = g1 * (float(x1) - 1.0) / float(d1) - g2 / float(d2)
    b[1, e] = g1 / float(d1) + g2 / float(d2) + g3 / float(d3)
    return sem, geo, a, b, ok


def occ_scal_ref(preds, label, mask=None, *, sem_scal_weight=1.0, geo_scal_weight=1.0, use_softmax=True, ignore_index=255,
                 empty_label=17, ignore_empty=False):
    """preds: list of [C, N] (or [1, C, N]) fp32 arrays.  Returns (loss, [grad [C, N] float64 per layer], sem [L], geo [L]):
    loss = (1/L) sum_l (sem_scal_weight sem_l + geo_scal_weight geo_l), NaN where the contract says so."""
    preds = [np.asarray(p).reshape(np.asarray(p).shape[-2], -1) for p in preds]
    L = len(preds)
    C, N = preds[0].shape
    label = np.asarray(label).reshape(-1).astype(np.int64)
    kept = np.ones(N, bool) if mask is None else np.asarray(mask).reshape(-1).astype(bool)
    if ignore_empty:
        kept = kept & (label != empty_label)
    bad = kept & ((label < 0) | (label >= C)) & (label != ignore_index)
    V = kept & (label != ignore_index) & (label >= 0) & (label < C)
    y = label[V]
    T = np.bincount(y, minlength=C)
    onehot = np.zeros((len(y), C))
    onehot[np.arange(len(y)), y] = 1.0
    total, grads, sems, geos, ok = 0.0, [], [], [], not bad.any()
    for x32 in preds:
        x = np.asarray(x32, dtype=np.float32).astype(np.float64).T[V]      # [|V|, C]
        if not np.all(np.isfinite(x)):
            ok = False
        if use_softmax:
            ex = np.exp(x - x.max(1, keepdims=True))
            p = ex / ex.sum(1, keepdims=True)
        else:
            p = x
        sem, geo, a, b, k = scal_terms(p.sum(0), (p * onehot).sum(0), T, empty_label)
        ok &= k
        gp = sem_scal_weight * (a[0][None] + b[0][None] * onehot) + geo_scal_weight * (a[1][None] + b[1][None] * onehot)
        if use_softmax:
            gp = p * (gp - (gp * p).sum(1, keepdims=True))
        g = np.zeros((N, C))
        g[V] = gp
        grads.append(g.T / L)
        sems.append(float(sem))
        geos.append(float(geo))
        total += sem_scal_weight * float(sem) + geo_scal_weight * float(geo)
    return (total / L if ok else np.nan), grads, sems, geos


def occ_loss_with_scal_ref(preds, label, mask=None, *, class_weights, sem_scal_weight=1.0, geo_scal_weight=1.0, **kw):
    """CE + Lovász (occ_loss_ref) plus the two terms: (loss, [grad [C, N]])."""
    base, bgrads = occ_loss_ref.occ_loss_ref(preds, label, mask, class_weights=class_weights, **kw)
    skw = {k: kw[k] for k in ("use_softmax", "ignore_index", "empty_label", "ignore_empty") if k in kw}
    scal, sgrads, _, _ = occ_scal_ref(preds, label, mask, sem_scal_weight=sem_scal_weight, geo_scal_weight=geo_scal_weight, **skw)
    return base + scal, [b + s for b, s in zip(bgrads, sgrads)]
