"""What ONE pass of the one-pass search (vectordb_amd/csrc/stream8_kernel.hpp, one_pass.hip) may leave behind, in integers: a plain numpy checker
for tests/test_one_pass_ref_cpu.py (fed with a numpy model of the pass and with planted faults) and tests/test_gpu_one_pass_pin.py (fed with
GpuIndex.one_pass_probe and GpuIndex.mirror_view(8, Q) of the same index and the same batch - the folded start values depend on the batch).

A *probe* is a dict: form (pieces, matrix, width, wide, prep_in_kernel, slots, waves, fold, rot, masked, wave_cap, chunk), k, raw_cnt [nq][waves],
raw [nq][waves][wave_cap] uint64 ((accumulator << 32) | row), table [nq][slots] int32, qstat [nq][4], kth [nq], T_final [nq].  A *view* is
tests/mirror_ref.py's.  `visible` is a bool [n] (None: every row): the deleted bitset, the int column test or a filter program evaluated with
@distance = 0, whichever the index carries.

Every check is an equality of integers or an inclusion of sets and holds for ANY interleaving of the wavefronts - the table only grows, so the
thresholds only tighten, and a row that reaches the final threshold reached every earlier one:

  (a) entries   every stored entry - all of a list whose count fits, the first wave_cap of one that overflowed - names a row < n that belongs to
                the wavefront that listed it ((row // chunk) % waves), no (query, row) pair is listed twice, and its accumulator is
                mirror_ref.acc8(view)[row, query]: the integer dot product of the view's codes plus the start value of this call (acc0b on a table
                that folds, else acc0).  In the clean form the view's q8 comes from query_prep8_kernel and the pass used stream8_prep_query's.
  (b) table     every filled slot j of query q holds the offer value - the accumulator, on a folding table minus TWICE the row's margin
                acc0b - acc0 - of a VISIBLE row with accumulator < 0x30000000 (not forced) and ((row * 2654435761 mod 2^32) >> 12) & (slots - 1) = j;
                kth is the slot of rank k - 1 under (value descending, slot ascending), INT32_MIN when fewer than k slots are filled.
  (e) T_final   the device's threshold against test_bound_math.threshold(upper_bound(kth)) evaluated in numpy fp32 from the view's maxima (scal8f
                on a folding table) and the PROBE's qstat.  Both are fp32 evaluations of the same real expression
                    T = floor((C - t) / u) - 2,  t = ub + margin + slack scale(ub) + 4 u,  ub = (C - u kth) + margin + 2 slack scale(C - u kth) + 4 u
                in which the compiler may contract a product and a sum into one fma and numpy may not.  On the path from the inputs to the quotient
                lie 17 roundings that are not damped by `slack`: (float) kth, u kth, C - .; the margin's product, sum and scaling, twice; three
                additions for ub and three for t; C - t; the division.  Each is at most 2^-24 of its result, and every result is at most
                M = the largest magnitude among C, u kth, ub, t and C - t.  The terms behind `slack` (the scales: at most 12 roundings each, one
                more for the product) add 25 x 2^-24 x 2 slack scale.  Two evaluations therefore differ by at most
                    allowance = ceil(2 (17 M + 50 slack scale) 2^-24 / u) + 1   accumulator units (+ 1: the floor),
                a few units for a query inside the table's range and thousands for one whose codes are clamped - where an accumulator unit is
                that much smaller against C.  This is asserted per query, and equality is what it amounts to where the allowance is 1.
                Largest difference observed on the MI355X over every case of tests/test_gpu_one_pass_pin.py: see OBSERVED below.
                Non-vacuity needs no number of its own: rows with acc >= T_final(device) are among those with acc >= T_restated - allowance.
  (c) complete  every row with accumulator >= T_final[q] - forced rows among them, visible or not - is in query q's lists, among the rows of
                wavefronts whose list did not overflow; and an overflowed list stores exactly wave_cap entries.
  (d) contract  independent of the formulas restated in (b) and (e): every visible row that is CERTAINLY among the k closest in fp64
                (tests/exact_ref.py: band() with the order-free fp32 bound) has accumulator >= T_final[q], and is listed.

A failure names query, row, accumulator, threshold, wavefront, the wavefront's chunk number, and the lane group (row % 16, K piece) or the slot."""
import math

import numpy as np

import mirror_ref as mr
import test_bound_math as bm

F = np.float32
S8_EMPTY = -(1 << 31)
FORCE_LIMIT = 0x30000000      # accumulators at or above it belong to forced rows (stream8_kernel.hpp S8_FORCE_LIMIT)
T_EVERYTHING = -(1 << 30)     # the threshold of a table with fewer than k filled slots
HASH = 2654435761
# largest |T_final(device) - T_restated| seen on the MI355X, and the allowance of that query (tests/test_gpu_one_pass_pin.py prints both per case)
OBSERVED = ("0 in most cases, 1 unit on some queries inside the grid (allowance 7 to 21 there: 520 and 1000 columns), 62 units on a folding table whose "
            "batch holds the query far outside the grid (allowance 1882); never beyond a tenth of the allowance")


def slot_of(rows, slots):
    rows = np.asarray(rows, np.uint64)
    return (((rows * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)) >> np.uint64(12) & np.uint64(slots - 1)).astype(np.int64)


def wave_of(rows, form):
    return (np.asarray(rows, np.int64) // form["chunk"]) % form["waves"]


def where(row, form):
    """what locates a row in the kernel"""
    row = int(row)
    return "wavefront %d, its chunk %d, row %% 16 = %d" % ((row // form["chunk"]) % form["waves"], row // (form["chunk"] * form["waves"]), row % 16)


def visible_mask(n, visible):
    return np.ones(n, bool) if visible is None else np.asarray(visible, bool)[:n]


def accumulators(view, probe):
    """acc8 with the start values this call used, [n][nq]"""
    return mr.acc8(view, folded=bool(probe["form"]["fold"]))


def int32_wrap(v):
    return ((np.asarray(v, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def offers(view, probe, acc):
    """what a row offers to the table: stream8_offer_value"""
    if not probe["form"]["fold"]:
        return acc
    n = view["n"]
    margin = np.asarray(view["acc0b"]).astype(np.int64)[:n] - np.asarray(view["acc0"]).astype(np.int64)[:n]
    return int32_wrap(acc - 2 * margin[:, None])   # (as the device's int arithmetic has it; only a forced row's wraps, and no forced row may offer)


def entries(probe):
    """(query, wavefront, position, row, accumulator) of every stored entry, as int64 arrays"""
    cap = probe["form"]["wave_cap"]
    cnt = np.asarray(probe["raw_cnt"], np.int64)
    raw = np.asarray(probe["raw"], np.uint64)
    valid = np.arange(cap)[None, None, :] < np.minimum(cnt, cap)[:, :, None]
    q, w, i = np.nonzero(valid)
    e = raw[q, w, i]
    rows = (e & np.uint64(0xFFFFFFFF)).astype(np.int64)
    accs = (e >> np.uint64(32)).astype(np.uint32).view(np.int32).astype(np.int64)
    return q, w, i, rows, accs


def _piece_hint(view, row, q, diff):
    """which 256-byte K piece of the row, left out or counted twice, explains an accumulator that is off by `diff`"""
    x = np.asarray(view["x8"][row]).astype(np.int64)
    y = np.asarray(view["q8"][q]).astype(np.int64)
    for p in range(view["d_pad"] // 256):
        dot = int((x[p * 256:(p + 1) * 256] * y[p * 256:(p + 1) * 256]).sum())
        if dot != 0 and diff == -dot:
            return " (= the row's dot without K piece %d)" % p
        if dot != 0 and diff == dot:
            return " (= K piece %d counted twice)" % p
    if "acc0b" in view and diff == int(view["acc0"][row]) - int(view["acc0b"][row]):
        return " (= started from acc0, not from the folded acc0b)"
    return ""


def check_entries(view, probe, acc):
    form, n = probe["form"], view["n"]
    q, w, i, rows, accs = entries(probe)
    bad = np.flatnonzero((rows < 0) | (rows >= n))
    assert len(bad) == 0, "(a) entries: query %d wavefront %d entry %d names row %d of a table of %d (accumulator %d)" % (
        q[bad[0]], w[bad[0]], i[bad[0]], rows[bad[0]], n, accs[bad[0]])
    bad = np.flatnonzero(wave_of(rows, form) != w)
    assert len(bad) == 0, "(a) entries: query %d row %d is in the list of wavefront %d, its rows belong to %s" % (q[bad[0]], rows[bad[0]], w[bad[0]], where(rows[bad[0]], form))
    key = q * n + rows
    uq, c = np.unique(key, return_counts=True)
    assert (c == 1).all(), "(a) entries: query %d lists row %d %d times (%s)" % (uq[c > 1][0] // n, uq[c > 1][0] % n, c.max(), where(uq[c > 1][0] % n, form))
    want = acc[rows, q]
    bad = np.flatnonzero(accs != want)
    if len(bad):
        b = bad[0]
        raise AssertionError("(a) entries: query %d row %d (%s): stored accumulator %d, the operands give %d, difference %d%s; %d of %d entries differ" % (
            q[b], rows[b], where(rows[b], form), accs[b], want[b], accs[b] - want[b], _piece_hint(view, int(rows[b]), int(q[b]), int(accs[b] - want[b])), len(bad), len(rows)))
    cnt = np.asarray(probe["raw_cnt"], np.int64)
    assert (cnt >= 0).all() and (cnt <= n).all(), "(a) entries: a wavefront counts more entries than the table has rows"


def kth_of(table_q, k):
    """slot of rank k - 1 under (value descending, slot ascending)"""
    t = np.asarray(table_q, np.int64)
    order = np.lexsort((np.arange(len(t)), -t))
    return int(t[order[k - 1]])


def check_table(view, probe, acc, visible=None):
    form, n, k = probe["form"], view["n"], probe["k"]
    slots = form["slots"]
    vis = visible_mask(n, visible)
    off = offers(view, probe, acc)
    slot = slot_of(np.arange(n), slots)
    by_slot = [np.flatnonzero(slot == j) for j in range(slots)]
    table = np.asarray(probe["table"], np.int64)
    assert table.shape == (acc.shape[1], slots), "(b) table: %s slots for %d queries of %d slots" % (table.shape, acc.shape[1], slots)
    for q in range(acc.shape[1]):
        elig = vis & (acc[:, q] < FORCE_LIMIT)
        for j in np.flatnonzero(table[q] != S8_EMPTY):
            g = int(table[q, j])
            rows = by_slot[j]
            if ((off[rows, q] == g) & elig[rows]).any():
                continue
            # ---- whose value is it then?
            same = np.flatnonzero(off[:, q] == g)
            raw = np.flatnonzero(acc[:, q] == g)
            once = np.flatnonzero(acc[:, q] - (acc[:, q] - off[:, q]) // 2 == g) if form["fold"] else np.array([], np.int64)   # g = accumulator - ONE margin
            if len(same) and (slot[same] == j).any():
                r = same[slot[same] == j][0]
                why = "the offer of row %d, which is %s" % (r, "forced (accumulator %d)" % acc[r, q] if acc[r, q] >= FORCE_LIMIT else "not visible")
            elif len(same):
                r = same[0]
                why = "the offer of row %d, whose slot is %d" % (r, slot[r])
            elif form["fold"] and len(raw):
                r = raw[0]
                why = "the ACCUMULATOR of row %d (slot %d), not its offer %d = accumulator - 2 x margin %d" % (r, slot[r], off[r, q], (acc[r, q] - off[r, q]) // 2)
            elif len(once):
                r = once[0]
                why = "accumulator - ONE margin of row %d (slot %d, accumulator %d, margin %d): its offer is %d" % (r, slot[r], acc[r, q], (acc[r, q] - off[r, q]) // 2, off[r, q])
            else:
                r = None
                why = "no row's offer"
            best = off[rows, q][elig[rows]].max(initial=S8_EMPTY)
            raise AssertionError("(b) table: query %d slot %d holds %d - %s; the largest offer a visible, unforced row of this slot can make is %d%s" % (
                q, j, g, why, best, "" if r is None else " (" + where(r, form) + ")"))
        want = kth_of(table[q], k)
        got = int(probe["kth"][q])
        assert got == want, "(b) table: query %d: kth = %d, the slot of rank %d (value descending, slot ascending) holds %d; %d of %d slots filled; slots in order: %s" % (
            q, got, k - 1, want, int((table[q] != S8_EMPTY).sum()), slots, np.lexsort((np.arange(slots), -table[q]))[max(0, k - 3):k + 2].tolist())


def restated_threshold(view, probe, q):
    """(T, allowance) of query q from the probe's kth and qstat and the view's maxima: test_bound_math in numpy fp32, and the fp32 allowance
    derived in the module's docstring"""
    form, metric = probe["form"], view["metric"]
    kth = int(probe["kth"][q])
    if kth == S8_EMPTY:
        return T_EVERYTHING, 0
    sc = np.asarray(view["scal8f" if form["fold"] else "scal8"], F)
    u = F(mr.key_unit(view))
    m = dict(scal=dict(e1max=sc[0], nxhmax=sc[1], xnmax=sc[2], rmax=sc[4], mun=sc[5], xcmax=sc[6]), u=u, s=F(2.0) if metric == 0 else F(1.0))
    s4 = np.asarray(probe["qstat"][q], F)
    qs = dict(qn2=s4[0], nq=s4[1], eq=s4[2], Cq=s4[3])
    slack = mr.rerank_slack(view["dim"])
    with np.errstate(over="ignore", invalid="ignore"):
        ub = bm.upper_bound(kth, qs, m, metric, slack)
        T = bm.threshold(ub, qs, m, metric, slack)
    # the magnitudes, in fp64
    C, u64 = float(s4[3]), float(u)
    margin = float(m["s"]) * (float(s4[1]) * float(sc[0]) + float(s4[2]) * float(sc[1]))
    dapx = C - u64 * kth

    def scale(thr):
        if metric == 0:
            return abs(thr) + margin + 2.0 * abs(C) + 2.0 * float(sc[4])
        return abs(thr) + margin + 1.0 + math.sqrt(float(s4[0])) * (math.sqrt(float(sc[2])) + float(sc[5])) + float(sc[5]) * float(sc[6]) + abs(C) + float(sc[4])
    ubr = dapx + margin + 2.0 * slack * scale(dapx) + 4.0 * u64
    t = ubr + margin + slack * scale(ubr) + 4.0 * u64
    M = max(abs(C), abs(u64 * kth), abs(dapx), abs(ubr), abs(t), abs(C - t))
    allowance = int(math.ceil(2.0 * (17.0 * M + 50.0 * slack * scale(ubr)) * mr.EPS / u64)) + 1
    return T, allowance


def check_threshold(view, probe):
    """returns (largest |device - restated| over the queries, that query's allowance, the smallest allowance of any query)"""
    worst, least = (0, 0), None
    for q in range(len(probe["kth"])):
        T, allow = restated_threshold(view, probe, q)
        got = int(probe["T_final"][q])
        if got in (T_EVERYTHING, mr.TQ_MAX8) or T in (T_EVERYTHING, mr.TQ_MAX8):   # (the clamps are exact)
            assert got == T, "(e) T_final: query %d: the device says %d, the restatement %d (kth %d)" % (q, got, T, probe["kth"][q])
            continue
        assert abs(got - T) <= allow, "(e) T_final: query %d: the device says %d, the restatement %d from kth %d: %d units apart, the fp32 operations allow %d" % (
            q, got, T, probe["kth"][q], got - T, allow)
        least = allow if least is None else min(least, allow)
        if abs(got - T) > worst[0]:
            worst = (abs(got - T), allow)
    return worst[0], worst[1], least


def listed_mask(probe, n):
    """[n][nq]: the row is among the stored entries of the query"""
    q, _, _, rows, _ = entries(probe)
    got = np.zeros((n, len(probe["kth"])), bool)
    got[rows, q] = True
    return got


def overflowed(probe):
    """[nq][waves]: the wavefront's list lost entries"""
    return np.asarray(probe["raw_cnt"], np.int64) > probe["form"]["wave_cap"]


def check_complete(view, probe, acc):
    form, n = probe["form"], view["n"]
    got = listed_mask(probe, n)
    ovf = overflowed(probe)
    wave = wave_of(np.arange(n), form)
    for q in range(acc.shape[1]):
        T = int(probe["T_final"][q])
        need = (acc[:, q] >= T) & ~ovf[q][wave]
        miss = np.flatnonzero(need & ~got[:, q])
        if len(miss):
            r = miss[0]
            forced = acc[r, q] >= FORCE_LIMIT
            raise AssertionError("(c) complete: query %d row %d (%s, rows %% 16 of all missing: %s) has accumulator %d >= T_final %d%s%s and is in no list; its wavefront counts %d entries; %d rows missing" % (
                q, r, where(r, form), sorted(set((miss % 16).tolist()))[:8], acc[r, q], T, " (exactly at the threshold)" if acc[r, q] == T else "", " (a forced row)" if forced else "",
                probe["raw_cnt"][q][wave[r]], len(miss)))
        # what a list that fits must hold, it holds exactly once (a): so its count is at least the rows of its wavefront that reach T_final
        cnt = np.asarray(probe["raw_cnt"][q], np.int64)
        least = np.bincount(wave[acc[:, q] >= T], minlength=form["waves"])
        bad = np.flatnonzero(cnt < least)
        assert len(bad) == 0, "(c) complete: query %d wavefront %d counts %d entries, %d of its rows reach T_final %d" % (q, bad[0] if len(bad) else -1, cnt[bad[0]] if len(bad) else -1, least[bad[0]] if len(bad) else -1, T)


def check_contract(view, probe, acc, ref, visible=None):
    """ref: exact_ref.Ref of the rows, the queries and the metric"""
    import exact_ref as er
    form, n, k = probe["form"], view["n"], probe["k"]
    vis = visible_mask(n, visible)
    B = ref.bound("free")
    got = listed_mask(probe, n)
    ovf = overflowed(probe)
    wave = wave_of(np.arange(n), form)
    for q in range(acc.shape[1]):
        must = er.band(ref, q, k, vis, B)[0]
        T = int(probe["T_final"][q])
        bad = np.flatnonzero(must & (acc[:, q] < T))
        assert len(bad) == 0, "(d) contract: query %d row %d (%s) is certainly among the %d closest (fp64 distance %r) and its accumulator %d is below T_final %d: the re-rank would never see it" % (
            q, bad[0] if len(bad) else -1, where(bad[0], form) if len(bad) else "", k, ref.d64[bad[0], q] if len(bad) else 0.0, acc[bad[0], q] if len(bad) else 0, T)
        bad = np.flatnonzero(must & ~got[:, q] & ~ovf[q][wave])
        assert len(bad) == 0, "(d) contract: query %d row %d (%s) is certainly among the %d closest and is in no list" % (q, bad[0] if len(bad) else -1, where(bad[0], form) if len(bad) else "", k)


def check_all(view, probe, visible=None, ref=None, acc=None):
    """(a), (b), (e), (c), (d) in the order in which each relies on the one before; returns a dict of figures for the log"""
    acc = accumulators(view, probe) if acc is None else acc
    assert acc.shape[1] == len(probe["kth"]) == len(probe["T_final"])
    check_entries(view, probe, acc)
    check_table(view, probe, acc, visible)
    worst = check_threshold(view, probe)
    check_complete(view, probe, acc)
    if ref is not None:
        check_contract(view, probe, acc, ref, visible)
    restated = [restated_threshold(view, probe, q)[0] for q in range(acc.shape[1])]
    return dict(entries=int(np.minimum(probe["raw_cnt"], probe["form"]["wave_cap"]).sum()), counted=int(np.asarray(probe["raw_cnt"]).sum()),
                at_or_above_T=int((acc >= np.asarray(probe["T_final"], np.int64)[None, :]).sum()), filled=int((np.asarray(probe["table"]) != S8_EMPTY).sum()),
                overflowed=int(overflowed(probe).sum()), T_device=[int(t) for t in probe["T_final"]], T_restated=restated, T_diff=worst[0], T_allowance=worst[1], T_least_allowance=worst[2])


def describe(probe, fig):
    """one line for the log"""
    f = probe["form"]
    kernel = "stream8m_kernel<%d, %d>" % (f["pieces"], f["width"]) if f["matrix"] else "stream8_kernel<%d, %d, %s%s>" % (
        f["pieces"], f["width"], "PREP" if f["prep_in_kernel"] else "false", ", WIDE" if f["wide"] else "")
    return "[one pass] %s slots %d waves %d fold %d rot %d masked %d | k %d queries %d | raw entries %d (counted %d, lists overflowed %d) rows >= T_final %d slots filled %d | T_final device %s restated %s (largest difference %d where %d are allowed; smallest allowance of a query %s)" % (
        kernel, f["slots"], f["waves"], f["fold"], f["rot"], f["masked"], probe["k"], len(probe["kth"]), fig["entries"], fig["counted"], fig["overflowed"], fig["at_or_above_T"],
        fig["filled"], fig["T_device"][:4], fig["T_restated"][:4], fig["T_diff"], fig["T_allowance"], fig["T_least_allowance"])
