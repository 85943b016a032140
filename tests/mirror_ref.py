"""A plain fp64 reference of what the mirrors of the flat matrix engine must hold and of what one filter pass must let through, for
tests/test_mirror_ref_cpu.py (fed with the numpy restatement of tests/test_bound_math.py) and tests/test_gpu_mirror_pin.py (fed with the
device's own arrays: GpuIndex.mirror_view / filter_pass).  Everything here is numpy float64 / int64; no constant is fitted to device output:
every allowance is the rounding of a counted number of fp32 operations, or an inflation the device code applies itself
(vectordb_amd/csrc/mirror_build.hip quant_mirror_kernel / query_prep8_kernel / fold8_kernel, device_common.hpp quant8 / stage_threshold8).

A *view* is a dict: x8 [n_pad][d_pad] int8, acc0, erow, hrow [n_pad], mu8 [d_pad], scal8 / scal8f [8], step, n, n_pad, d_pad, dim, metric,
rot, rot_w, fold (+ sp8 when rotated), and for a batch of queries q8 [nq][d_pad], qstat [nq][4] (+ acc0b, qmax when the table folds)."""
import numpy as np

import test_bound_math as bm

F = np.float32
EPS = 2.0 ** -24          # unit roundoff of fp32
ACC_PAD = -(1 << 30)      # start value of padding rows and of forced rows before the fold
ACC_FORCE = bm.ACC_FORCE
TQ_MAX8 = bm.TQ_MAX


def rerank_slack(dim):
    """mirror.hpp rerank_slack: the relative fp32 allowance of a d-term sum (64 lanes x d/64 sequential fmas + a 6-level tree), doubled"""
    return max(8e-6, 2.0 * (3.0 * (((dim + 63) // 64 * 64) / 64.0 + 6.0) + 6.0) * EPS)


def key_unit(view):
    """u = |s| step^2 as the host computes it in fp32 (mirror.hpp key_unit8)"""
    s = F(2.0) if view["metric"] == 0 else F(1.0)
    return float(s * F(view["step"]) * F(view["step"]))


def frame(view, X):
    """fp64 image of rows (or queries) in the view's frame, [len][cols]: x itself, or R x (tests/test_bound_math.py rotate_rows)"""
    X = np.asarray(X, np.float64)
    if view["rot"]:
        Y = bm.rotate_rows(X)
        assert Y.shape[1] == view["rot_w"]
        if "sp8" in view:   # the device's table is the restatement's
            src, neg = bm.rotation_table(view["rot_w"])
            sp = np.asarray(view["sp8"][:view["rot_w"]]).astype(np.int64) & 0xFFFFFFFF
            assert np.array_equal(sp & 0x7FFFFFFF, src) and np.array_equal((sp >> 31) != 0, neg), "rotation table differs"
        return Y
    return X


def cols(view):
    return view["rot_w"] if view["rot"] else view["dim"]


def centred(view, X):
    """x' = x - mu (rotated frame: R x - mu) in fp64, and |x| in the frame"""
    Y = frame(view, X)
    return Y - np.asarray(view["mu8"][:cols(view)], np.float64), np.sqrt((Y * Y).sum(1))


def _codes_ok(view, xc, xnorm, codes, what):
    step = float(view["step"])
    q = xc / step
    # the device forms the quotient as fl(fl(x - mu) * fl(1 / step)): three fp32 roundings, each <= 2^-24 relative, on a value whose
    # magnitude matters only below the clamp (|quotient| >= 256 rounds beyond +-127 whatever the roundings do); rotated frame: + the fp64
    # transform's remainder the code itself allows for, 1e-12 |x|
    r = 3.0 * EPS * (1.0 + 2.0 * EPS) * np.minimum(np.abs(q), 256.0)
    if view["rot"]:
        r = r + 1e-12 * xnorm[:, None] / step
    err = np.abs(np.clip(q, -127.0, 127.0) - codes[:, :xc.shape[1]])
    bad = np.argwhere(err > 0.5 + r)
    assert len(bad) == 0, "%s: %d codes are not a rounding of (x - mu) / step; first (row, column) %s: quotient %r code %d" % (
        what, len(bad), bad[0], q[tuple(bad[0])], codes[tuple(bad[0])])
    assert np.abs(codes).max(initial=0) <= 127, what + ": code beyond +-127"
    assert not codes[:, xc.shape[1]:].any(), what + ": nonzero code in a padding column"


def check_codes(view, X):
    n = view["n"]
    assert len(X) == n
    x8 = np.asarray(view["x8"]).astype(np.int64)
    xc, xnorm = centred(view, X)
    _codes_ok(view, xc, xnorm, x8[:n], "rows")
    assert not x8[n:].any(), "padding rows carry codes"
    assert (np.asarray(view["acc0"])[n:] == ACC_PAD).all(), "padding rows must never pass (acc0 = -2^30)"
    if "q8" in view and "Q" in view:
        qc, qnorm = centred(view, view["Q"])
        _codes_ok(view, qc, qnorm, np.asarray(view["q8"]).astype(np.int64), "queries")


def row_reference(view, X):
    """fp64: x', residual norm, grid norm, R, per row"""
    n, step = view["n"], float(view["step"])
    xc, xnorm = centred(view, X)
    xi = np.asarray(view["x8"])[:n, :xc.shape[1]].astype(np.float64)
    res = np.sqrt(((xc - step * xi) ** 2).sum(1))
    grid = np.sqrt(((step * xi) ** 2).sum(1))
    xcn = np.sqrt((xc * xc).sum(1))
    mu = np.asarray(view["mu8"][:xc.shape[1]], np.float64)
    R = (xc * xc).sum(1) if view["metric"] == 0 else -(xc * mu).sum(1)
    return dict(xc=xc, xnorm=xnorm, res=res, grid=grid, xcn=xcn, R=R)


def acc0_allowance(view):
    """accumulator units by which acc0 may fall short of -R / u: the share of slack * scale that stage_threshold8 reserves for the fp32
    evaluation of R, divided by u.  L2: R = |x'|^2, a sum of non-negative terms - the 2 rmax term.  IP / COSINE: R = -mu . x' is a d-term
    sum that CANCELS: its rounding scales with the sum of its terms' magnitudes, <= |mu| |x'|, not with |R|, and the scale carries
    mun * xcmax next to rmax for exactly that (on rows far from the origin |R| is a thousandth of |mu| |x'|: the rmax term alone rejects the
    restatement the CPU suite proves sound)."""
    sc = np.asarray(view["scal8"], np.float64)
    share = 2.0 * sc[4] if view["metric"] == 0 else sc[4] + sc[5] * sc[6]
    return rerank_slack(view["dim"]) * share / key_unit(view)


def check_row_constants(view, X, metric):
    assert metric == view["metric"]
    n = view["n"]
    ref = row_reference(view, X)
    u = key_unit(view)
    S = rerank_slack(cols(view))   # fp32 summation bound of a d-term sum, relative
    erow, hrow = np.asarray(view["erow"], np.float64)[:n], np.asarray(view["hrow"], np.float64)[:n]
    acc0 = np.asarray(view["acc0"]).astype(np.int64)[:n]
    forced = np.isinf(erow)
    assert int(forced.sum()) == view["forced_rows"], (int(forced.sum()), view["forced_rows"])
    assert (acc0[forced] == ACC_PAD).all(), "a forced row must never be selected on approximate keys"
    v = -ref["R"] / u
    assert (np.abs(v[forced]) >= 536870912.0 * (1.0 - 1e-5)).all(), "a row is forced whose constant fits the accumulator"
    ok = ~forced
    # ---- soundness: no tolerance on the norms (the code inflates them itself); acc0: less only the fp32 evaluation of R
    bad = np.flatnonzero(ok & ~(erow >= ref["res"]))
    assert len(bad) == 0, "erow below the fp64 residual norm on %d rows; row %d: %r < %r" % (len(bad), bad[0], erow[bad[0]], ref["res"][bad[0]])
    bad = np.flatnonzero(~(hrow >= ref["grid"]))
    assert len(bad) == 0, "hrow below the fp64 norm of the grid point on %d rows; row %d: %r < %r" % (len(bad), bad[0], hrow[bad[0]], ref["grid"][bad[0]])
    allow = acc0_allowance(view)
    bad = np.flatnonzero(ok & ~(acc0 >= v - allow))
    assert len(bad) == 0, "acc0 below -R / u - %.2f on %d rows; row %d: %d < %r" % (allow, len(bad), bad[0], acc0[bad[0]], v[bad[0]])
    # ---- tightness: the code's own inflation (x 1.00001, + 1.2e-7 |x'|, rotated + 1e-12 |x|; ceil + 1), the rounding of x - mu that the
    # device's residual is taken from (2^-24 |x'|), and the summation bound
    hi_e = (ref["res"] + EPS * ref["xcn"]) * 1.00001 * (1.0 + S) + 1.2e-7 * ref["xcn"] * (1.0 + S) + (1e-12 * ref["xnorm"] if view["rot"] else 0.0)
    bad = np.flatnonzero(ok & ~(erow <= hi_e))
    assert len(bad) == 0, "erow looser than the code's own inflation on %d rows; row %d: %r > %r" % (len(bad), bad[0], erow[bad[0]], hi_e[bad[0]])
    hi_h = ref["grid"] * 1.00001 * (1.0 + S)
    bad = np.flatnonzero(~(hrow <= hi_h))
    assert len(bad) == 0, "hrow looser than the code's own inflation on %d rows; row %d: %r > %r" % (len(bad), bad[0], hrow[bad[0]], hi_h[bad[0]])
    bad = np.flatnonzero(ok & ~(acc0 <= v + allow + 2.0))
    assert len(bad) == 0, "acc0 above -R / u + %.2f + 2 on %d rows; row %d: %d > %r" % (allow, len(bad), bad[0], acc0[bad[0]], v[bad[0]])
    # ---- the table's maxima bound every tested row (they enter the thresholds)
    sc = np.asarray(view["scal8"], np.float64)
    if ok.any():
        assert sc[0] >= erow[ok].max() and sc[1] >= hrow[ok].max() and sc[4] >= np.abs(ref["R"][ok]).max() * (1.0 - S), "a maximum is below a row's value"
        assert sc[0] == erow[ok].max() and sc[1] == hrow[ok].max(), "a maximum is above every row's value"
    assert sc[6] >= sc[0] + sc[1] - 1e-6 * (sc[0] + sc[1])
    scf = np.asarray(view["scal8f"], np.float64)
    assert scf[0] == 0 and scf[1] == 0 and np.array_equal(scf[2:7], sc[2:7]), "scal8f is scal8 with the two margin entries zeroed"
    # ---- the batch's folded start values
    if "acc0b" in view:
        acc0b = np.asarray(view["acc0b"]).astype(np.int64)
        assert (acc0b[n:] == ACC_PAD).all(), "padding rows of the folded start values"
        qn, eq = (float(t) for t in np.asarray(view["qmax"], np.uint32).view(np.float32))
        qs = np.asarray(view["qstat"], np.float32)
        assert F(qn) == qs[:, 1].max() and F(eq) == qs[:, 2].max(), "qmax is not the batch's largest query norms"
        s = 2.0 if metric == 0 else 1.0
        with np.errstate(invalid="ignore", over="ignore"):
            marg = s * (qn * erow + eq * hrow) / u
        force = forced | ~(marg < 536870912.0 * (1.0 - 1e-5))
        assert (acc0b[:n][forced] == ACC_FORCE).all(), "a forced row must start at ACC_FORCE after the fold"
        live = acc0b[:n] != ACC_FORCE
        assert not (~live & ~force).any(), "a row starts at ACC_FORCE whose margin fits the accumulator"
        add = (acc0b[:n] - acc0)[live]
        m = marg[live]
        # fold8_kernel: ceilf(fl(s * fl(fl(qn * e) + fl(eq * h)) * fl(1 / u))) + 1 - six fp32 roundings under the ceil
        assert (add >= m * (1.0 - 6.0 * EPS) + 1.0).all(), "a folded start value carries less than the row's margin"
        assert (add <= m * (1.0 + 6.0 * EPS) + 2.0).all(), "a folded start value carries more than the row's margin + the ceil"


def check_query_constants(view, Q, metric):
    assert metric == view["metric"]
    step = float(view["step"])
    qc, qnorm = centred(view, Q)
    qi = np.asarray(view["q8"])[:, :qc.shape[1]].astype(np.float64)
    qs = np.asarray(view["qstat"], np.float64)
    S = rerank_slack(cols(view))
    qcn = np.sqrt((qc * qc).sum(1))
    res = np.sqrt(((qc - step * qi) ** 2).sum(1))
    mu = np.asarray(view["mu8"][:qc.shape[1]], np.float64)
    Y = qc + mu
    qmu = (Y * mu).sum(1)
    C = (qc * qc).sum(1) if metric == 0 else (1.0 - qmu if metric == 1 else -qmu)
    assert (np.abs(qs[:, 0] - qnorm ** 2) <= S * qnorm ** 2).all(), "qstat[0] is not |q|^2"
    # soundness: the two norms the margin multiplies
    bad = np.flatnonzero(~(qs[:, 1] >= qcn))
    assert len(bad) == 0, "qstat[1] below |q - mu| for query %d: %r < %r" % (bad[0], qs[bad[0], 1], qcn[bad[0]])
    bad = np.flatnonzero(~(qs[:, 2] >= res))
    assert len(bad) == 0, "qstat[2] below the fp64 residual norm for query %d: %r < %r" % (bad[0], qs[bad[0], 2], res[bad[0]])
    # tightness: x 1.000001 / x 1.00001 + 1.2e-7 |q'| (+ 1e-12 |q|), the rounding of q - mu, the summation bound
    assert (qs[:, 1] <= qcn * 1.000001 * (1.0 + S)).all(), "qstat[1] looser than the code's own inflation"
    hi = (res + EPS * qcn) * 1.00001 * (1.0 + S) + 1.2e-7 * qcn * (1.0 + S) + (1e-12 * qnorm if view["rot"] else 0.0)
    assert (qs[:, 2] <= hi).all(), "qstat[2] looser than the code's own inflation"
    # C[q] within the share of slack * scale that stage_threshold8 reserves for it: L2 2 |C|; otherwise 1 + |q| |mu| + |C|
    slack = rerank_slack(view["dim"])
    share = 2.0 * np.abs(C) if metric == 0 else 1.0 + qnorm * np.sqrt((mu * mu).sum()) + np.abs(C)
    bad = np.flatnonzero(~(np.abs(qs[:, 3] - C) <= slack * share))
    assert len(bad) == 0, "qstat[3] is not C[q] for query %d: %r vs %r" % (bad[0], qs[bad[0], 3], C[bad[0]])


def start8(view, folded=None):
    """the accumulators' start values of a pass: the batch's folded ones in exact mode on a table that folds, else acc0"""
    folded = bool(view["fold"]) if folded is None else folded
    return np.asarray(view["acc0b" if folded else "acc0"]).astype(np.int64)[:view["n"]]


def acc8(view, folded=None):
    """x8 . q8 + start value, exact integers [n][nq]: |dot| <= 127^2 d_pad < 2^27 is exact in a float64 BLAS product (in blocks of rows: the
    float64 image of a quarter of a million rows is gigabytes)"""
    n = view["n"]
    q = np.asarray(view["q8"]).astype(np.float64).T
    x8 = np.asarray(view["x8"])
    out = np.empty((n, q.shape[1]), np.int64)
    for r0 in range(0, n, 32768):
        out[r0:r0 + 32768] = np.rint(x8[r0:min(n, r0 + 32768)].astype(np.float64) @ q)
    return out + start8(view, folded)[:, None]


def explain_pairs(pairs, acc, T, limit=6):
    """(row, query) pairs a tile decided wrongly, with what locates them in the kernel"""
    return "; ".join("query %d row %d (tile %d, row %% 32 = %d, query column %d) accumulator %s threshold %s" % (q, r, r // 256, r % 32, q % 64, acc[r, q], T[q])
                     for r, q in sorted(pairs)[:limit])


def check_pass(acc, lo, hi, T, cap, cnt, lists, what=""):
    """what ONE pass over rows [lo, hi) returned (cnt [nq]; lists: per query the row ids it listed) against the reference accumulators
    acc [n][nq] and thresholds T [nq] (a row passes iff acc >= T): the counts exactly; every list duplicate-free, inside [lo, hi) and inside
    the reference set; equal to it as a set when the count fits the cap, else exactly cap entries"""
    T = np.asarray(T)
    want = acc[lo:hi] >= T[None, :]
    cnt = np.asarray(cnt, np.int64)
    bad = np.flatnonzero(cnt != want.sum(0))
    assert len(bad) == 0, "%s: query %d reports %d rows, the reference %d (threshold %s)" % (what, bad[0], cnt[bad[0]], want[:, bad[0]].sum(), T[bad[0]])
    for j, rows in enumerate(lists):
        rows = np.asarray(rows, np.int64)
        assert len(np.unique(rows)) == len(rows), "%s: query %d lists a row twice" % (what, j)
        out = rows[(rows < lo) | (rows >= hi)]
        assert len(out) == 0, "%s: query %d lists row %d outside [%d, %d)" % (what, j, out[0] if len(out) else -1, lo, hi)
        ref = lo + np.flatnonzero(want[:, j])
        extra = np.setdiff1d(rows, ref)
        assert len(extra) == 0, "%s: reported below the threshold: %s" % (what, explain_pairs([(int(r), j) for r in extra], acc, T))
        if cnt[j] <= cap:
            miss = np.setdiff1d(ref, rows)
            assert len(miss) == 0, "%s: not reported: %s" % (what, explain_pairs([(int(r), j) for r in miss], acc, T))
        else:
            assert len(rows) == cap, "%s: query %d lists %d rows of a full list of %d" % (what, j, len(rows), cap)


def dist64(X, Q, metric):
    """fp64 distances [n][nq], term by term for L2 (no cancellation)"""
    X, Q = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    if metric == 0:
        return np.stack([((X - q) ** 2).sum(1) for q in Q], axis=1)
    d = X @ Q.T
    return 1.0 - d if metric == 1 else -d


def must_pass(view, X, Q, metric, thr):
    """[n][nq]: pairs the library's contract obliges a pass with threshold distances `thr` [nq] to report"""
    return dist64(X, Q, metric) <= np.asarray(thr, np.float64)[None, :]


def thresholds8(view, thr, folded=None, approx=False):
    """the restatement's T for distances thr [nq] from the VIEW's constants (test_bound_math.threshold)"""
    folded = bool(view["fold"]) if folded is None else folded
    sc = np.asarray(view["scal8"], F)
    m = dict(scal=dict(e1max=sc[0], nxhmax=sc[1], xnmax=sc[2], rmax=sc[4], mun=sc[5], xcmax=sc[6]), u=F(key_unit(view)),
             s=F(2.0) if view["metric"] == 0 else F(1.0))
    out = []
    for t, qs in zip(np.asarray(thr, F), np.asarray(view["qstat"], F)):
        out.append(bm.threshold(F(t), dict(qn2=qs[0], nq=qs[1], eq=qs[2], Cq=qs[3]), m, view["metric"], rerank_slack(view["dim"]), folded=folded or approx))
    return np.array(out, np.int64)


# ------------------------------------------------------------------------------------------------ fp16 operands
def approx16(view):
    """start value + fp64 dot of the fp16 operands, [n][nq]: the accumulator the tile compares (a row passes iff it is >= T / s)"""
    n = view["n"]
    return np.asarray(view["start"], np.float64)[:n, None] + np.asarray(view["xh"])[:n].astype(np.float64) @ np.asarray(view["qh"]).astype(np.float64).T


def band16(view):
    """|fp32 accumulation - exact| <= gamma |qh| |xh|, gamma = 4 d_pad 2^-24 (mirror_build.hip ensure_mirror), [n][nq]"""
    n = view["n"]
    gamma = 4.0 * view["d_pad"] * EPS
    xn = np.sqrt((np.asarray(view["xh"])[:n].astype(np.float64) ** 2).sum(1))
    qn = np.sqrt((np.asarray(view["qh"]).astype(np.float64) ** 2).sum(1))
    return gamma * xn[:, None] * qn[None, :]


def host_view16(X, Q, metric):
    """the fp16 view from the rows alone (X.astype(float16) needs no device): for conditions asserted before the device is asked"""
    n, d = X.shape
    d_pad = (d + 63) // 64 * 64
    xh = np.zeros((n, d_pad), np.float16)
    xh[:, :d] = X
    qh = np.zeros((len(Q), d_pad), np.float16)
    qh[:, :d] = Q
    start = -0.5 * (X.astype(np.float64) ** 2).sum(1) if metric == 0 else np.zeros(n)
    return dict(n=n, d_pad=d_pad, xh=xh, qh=qh, start=start, metric=metric)


# ------------------------------------------------------------------------------------------------ a view from the restatement
def restated_view(X, Q, metric, rot=False, mu=None, step=None):
    """the view the numpy restatement of tests/test_bound_math.py makes of rows X and queries Q (mirror / mirror_rot, query / query_rot, fold)"""
    n, d = X.shape
    W = bm.d_pad8_of(d)
    d_pad = max(512, W)
    n_pad = (n + 255) // 256 * 256
    m = (bm.mirror_rot if rot else bm.mirror)(X, metric, mu=mu, step=step)
    c = W if rot else d
    x8 = np.zeros((n_pad, d_pad), np.int8)
    x8[:n, :c] = m["xi"]
    pad = lambda v, fill, dt: np.concatenate([np.asarray(v, dt), np.full(n_pad - n, fill, dt)])
    mu8 = np.zeros(d_pad, F)
    mu8[:c] = m["mu"]
    sc = m["scal"]
    scal8 = np.array([sc["e1max"], sc["nxhmax"], sc["xnmax"], 0.0, sc["rmax"], sc["mun"], sc["xcmax"], 0.0], F)
    scal8f = scal8.copy()
    scal8f[:2] = 0
    ok = ~m["forced"]
    fold = bool(m["forced"].any() or (ok.any() and sc["e1max"] > F(1.5) * m["erow"][ok].min()))
    view = dict(bits=8, metric=metric, dim=d, n=n, n_pad=n_pad, d_pad=d_pad, rot=int(rot), rot_w=W, fold=int(fold), step=float(m["step"]),
                forced_rows=int(m["forced"].sum()), x8=x8, acc0=pad(m["acc0"], ACC_PAD, np.int32), erow=pad(m["erow"], 0, F), hrow=pad(m["hrow"], 0, F),
                mu8=mu8, scal8=scal8, scal8f=scal8f, usable=1, restated=m)
    if Q is not None:
        per = [(bm.query_rot if rot else bm.query)(np.asarray(q, F), m, metric) for q in Q]
        q8 = np.zeros((len(Q), d_pad), np.int8)
        q8[:, :c] = np.array([qi for qi, _ in per])
        view["q8"] = q8
        view["qstat"] = np.array([[qs["qn2"], qs["nq"], qs["eq"], qs["Cq"]] for _, qs in per], F)
        view["Q"] = np.asarray(Q, F)
        if fold:
            view["acc0b"] = pad(bm.fold(m, [qs for _, qs in per]), ACC_PAD, np.int32)
            view["qmax"] = np.array([max(qs["nq"] for _, qs in per), max(qs["eq"] for _, qs in per)], F).view(np.uint32)
    return view
