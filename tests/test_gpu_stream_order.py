"""WHEN a call reads its inputs and writes its outputs, on a caller's stream with the device still busy (tests/stream_gate.py: gate, window, the
cases and their vacuity condition).  What the calls compute is pinned elsewhere; every test here runs on s = torch.cuda.Stream() with
ix.set_stream(s.cuda_stream), queues a gate of plain torch work in front of the call, and ends in ONE stream.synchronize():

  a  every engine reads its device queries (lists, attribute rows) at its place in the stream: they hold the real values only there;
  b  eight calls back to back on one index, scratch regrowing under pending work, each equal to the same call made alone - on the caller's stream
     and on the index's own; set_stream drains the stream it leaves;
  c  a borrowed device bitset / int column is read in place: changed on the stream between two searches, never installed again;
  d  a HOST array has been read when the call returns (the rule of set_deleted, made general): it is overwritten from the host straight after;
  e  the free functions with a stream= argument.

Tables of small integers: ids, distance bits and counts are compared with no tolerance, against numpy (stream_gate.topk_np), exact_ref.check_exact
and the same call made alone with NumPy arrays and a sync.  Every case prints its issue time and gate length (`stream-gate: ...`) and one line
`stream-order: ...` that says whether the call returned behind the gate; the two calls documented asynchronous must have."""
import os

import numpy as np
import pytest

import exact_ref as xr
import stream_gate as sg
from helpers import data

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import vectordb_amd
    from vectordb_amd.build import build
    build()
    return vectordb_amd


class Env:
    def __init__(self, amd):
        import torch
        self.amd, self.torch = amd, torch
        self.s = torch.cuda.Stream()
        self.ix = {}
        sg.calibrate()

    def index(self, tab):
        if tab not in self.ix:
            X = sg.table(tab)
            ix = self.amd.GpuIndex(X.shape[1], 0)
            ix.attach_rows(X)
            ix.set_stream(self.s.cuda_stream)
            self.ix[tab] = ix
        return self.ix[tab]

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def full(self, shape, dtype):
        return self.torch.full(shape, sg.FILL, dtype=getattr(self.torch, dtype), device="cuda")

    def outs(self, nq, k, totals=False):
        o = [self.full((nq, k), "int64"), self.full((nq, k), "float32"), self.full((nq,), "int32")]
        return o + [self.full((nq,), "int64")] if totals else o

    def sync(self):
        self.torch.cuda.synchronize()


@pytest.fixture(scope="module")
def env(amd):
    e = Env(amd)
    yield e
    for ix in e.ix.values():
        ix.close()


ASYNC_WHY = ("%s returned with the stream idle (issue %.3f ms, gate %.3f ms).  Look at the ISSUE time: far above the ~0.1 ms of a few launches means the "
             "call waits for the device - a hidden sync; if it is small, look at the GATE: it ran out before the call returned and is too short")


def windowed(env, case, call, make_outs, inputs=None, asynchronous=False, alone=None, what="", prepare=None):
    """the pattern of (a) and (e).  call(tensors, outs): the call under test on device inputs; inputs: which arrays of case['real'] are windowed
    (default all); alone: the same call's answer made alone with NumPy arrays; prepare(tensors): once, before anything runs (a borrowed buffer is
    installed).  Returns (what the call wrote, behind)."""
    torch, s = env.torch, env.s
    name = case["name"] + what
    sg.check_case(case)
    idx = range(len(case["real"])) if inputs is None else inputs
    real = [env.dev(case["real"][i]) for i in idx]
    decoy = [env.dev(case["decoy"][i]) for i in idx]
    dst = [r.clone() for r in real]
    env.sync()
    if prepare:
        prepare(dst)

    def issue():      # (the real inputs again first: a call may work in place)
        for t, v in zip(dst, real):
            t.copy_(v)
        call(dst, make_outs())
    with torch.cuda.stream(s):      # the gate's length: the call once warm, once timed, on the real inputs, with no gate
        ms = sg.gate_for(name, issue, s)
    outs = make_outs()
    env.sync()
    sg.starts_as_fill([o.cpu().numpy() for o in outs], name)
    with sg.window(s, dst, real, decoy, ms) as w:
        with torch.cuda.stream(s):
            call(dst, outs)
        w.returned(*outs)
    s.synchronize()
    got = w.numpy()
    print("stream-order: %-58s returned behind the gate: %s" % (name, w.behind))
    i = case["names"].index("ids") if "ids" in case["names"] else 0
    why = "%s: the call read %s (by first ids)" % (name, sg.took(got[i], case["want"][i], case["want_decoy"][i]))
    sg.same(got, case["want"], why + " - against numpy", case["names"])
    if alone is not None:
        sg.same(got, alone, why + " - against the same call made alone", case["names"])
    if asynchronous:
        assert w.behind, ASYNC_WHY % (name, ms / 4, ms)
    return got, w.behind


def exact_sample(case, got, X, Q):
    """exact_ref.check_exact on up to 20 of the queries"""
    nq = len(Q)
    sample = np.arange(0, nq, max(1, nq // 20))[:20]
    xr.check_exact(got[0][sample], got[1][sample], got[2][sample], X, None, 0, case["k"], ref=sg.int_ref(X, Q[sample]), what=case["name"])


# ------------------------------------------------------------------------------------------------ a. every engine reads its queries at its place
def search_windowed(env, case, what="", **kw):
    amd, ix = env.amd, env.index(case["tab"])
    Q = case["real"][0]
    nq, k = len(Q), case["k"]
    kw.setdefault("mode", amd.MODE_FLAT)
    alone = ix.search(Q, k, **kw)
    ix.synchronize()
    got, _ = windowed(env, case, lambda t, o: ix.search(t[0], k, out=tuple(o), **kw), lambda: env.outs(nq, k), alone=alone, what=what)
    exact_sample(case, got, sg.table(case["tab"]), Q)
    return ix.stats()


@pytest.mark.parametrize("nq,k", [(1, 10), (70, 100), (3, 1500)])
def test_a_stream_engine_reads_queries_in_place(env, nq, k):
    """k = 1500: the result pages beyond 1024"""
    st = search_windowed(env, sg.search_case("A", nq, k), flat_engine=env.amd.FLAT_STREAM)
    assert st["main_kernel_bits"] == 32, st


@pytest.mark.parametrize("engine,bits", [("FLAT_MFMA", 16), ("FLAT_MFMA_I8", 8)])
def test_a_matrix_engines_read_queries_in_place(env, engine, bits):
    st = search_windowed(env, sg.search_case("B", 300, 10), what=" " + engine, flat_engine=getattr(env.amd, engine))
    assert st["main_kernel_bits"] == bits, st


@pytest.mark.parametrize("nq", [1, 8])
def test_a_one_pass_form_reads_queries_in_place(env, nq):
    st = search_windowed(env, sg.search_case("B", nq, 10, seed=21), what=" one pass", flat_engine=env.amd.FLAT_MFMA_I8)
    assert st["one_pass"] == 1, st


@pytest.mark.parametrize("T", [1, 4])
def test_a_graph_walk_reads_queries_in_place(env, T):
    """the golden graph's table is U[0,1) and a walk is not an exact search: the answer held to is the same call's made alone, bit for bit - for
    the real queries and, for the vacuity condition, for the decoys"""
    amd = env.amd
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph2000x32.npz"))
    X, Qr, Qd = data(2000, 32, 42), data(8, 32, 43), data(8, 32, 44)
    near = lambda Q: xr.dist64(X, Q, 0).argmin(axis=0)      # noqa: E731
    sg.differ_first(near(Qr), near(Qd), "graph walk: exact first ids")
    ix = amd.GpuIndex(32, 0)
    try:
        ix.attach_rows(X)
        ix.set_graph(z["off"].astype(np.int64), z["nbr"].astype(np.int64), int(z["nav"]))
        ix.set_stream(env.s.cuda_stream)
        kw = dict(mode=amd.MODE_GRAPH, intra_threads=T)
        want, want_decoy = ix.search(Qr, 10, **kw), ix.search(Qd, 10, **kw)
        ix.synchronize()
        case = dict(name="graph walk T %d nq 8 k 10" % T, real=(Qr,), decoy=(Qd,), want=want, want_decoy=want_decoy, names=("ids", "dist", "counts"))
        windowed(env, case, lambda t, o: ix.search(t[0], 10, out=tuple(o), **kw), lambda: env.outs(8, 10))
    finally:
        ix.close()


@pytest.mark.parametrize("tab,engine", [("A", "stream"), ("B", "mfma_i8")])
def test_a_search_range_reads_queries_in_place(env, tab, engine):
    """one query beyond the cap (RANGE_TOPK: flat_stream behind a host sync), one complete; the radii are a host array throughout"""
    ix = env.index(tab)
    case = sg.range_case(tab)
    Q, radius = case["real"]
    cap = case["cap"]
    alone = ix.search_range(Q, radius, cap, flat_engine=engine)
    ix.synchronize()
    windowed(env, case, lambda t, o: ix.search_range(t[0], radius, cap, flat_engine=engine, out=tuple(o)), lambda: env.outs(len(Q), cap, totals=True),
             inputs=[0], alone=alone, what=" " + engine)
    st = ix.stats()
    assert st["overflow_queries"] >= 1, st
    if engine == "mfma_i8":
        assert st["main_kernel_bits"] == 8, st


@pytest.mark.parametrize("shared", [True, False])
def test_a_search_among_reads_queries_and_lists_in_place(env, shared):
    """device queries AND a device id list, both valid in the call's window only; documented asynchronous"""
    ix = env.index("A")
    case = sg.among_case("A", 6, 10, shared)
    Q, L = case["real"]
    alone = ix.search_among(Q, L, 10, offsets=case["offsets"])
    ix.synchronize()
    windowed(env, case, lambda t, o: ix.search_among(t[0], t[1], 10, offsets=case["offsets"], out=tuple(o)), lambda: env.outs(len(Q), 10),
             asynchronous=True, alone=alone)


def test_a_select_reads_attribute_rows_in_place(env):
    """device attribute rows under a program filter (borrowed: used in place), device outputs; documented asynchronous"""
    ix = env.index("A")
    case = sg.select_case("A")
    skip, limit = case["skip"], case["limit"]
    try:
        ix.set_filter_program(sg.SELECT_PROG, case["real"][0].reshape(-1, 1))
        ids, total = ix.select(skip, limit)
        alone = (np.concatenate([ids, np.full(limit - len(ids), sg.FILL, np.int64)]), np.array([len(ids), total], np.int64))
        case = dict(case, real=(case["real"][0].reshape(-1, 1),), decoy=(case["decoy"][0].reshape(-1, 1),))
        windowed(env, case, lambda t, o: ix.select(skip, limit, out=tuple(o)), lambda: [env.full((limit,), "int64"), env.full((2,), "int64")],
                 asynchronous=True, alone=alone, prepare=lambda t: ix.set_filter_program(sg.SELECT_PROG, t[0], stride=4))      # (installed ONCE: the window's tensor)
    finally:
        ix.set_filter_program(None)


# ------------------------------------------------------------------------------------------------ b. back-to-back calls do not tread on each other
def back_to_back_calls(env, ix):
    """the eight calls of (b) on table A under the program filter `attribute > 5` -> [(name, device call(outs), make_outs, numpy call, numpy answer)]"""
    amd = env.amd
    X = sg.table("A")
    n = len(X)
    attr = sg.select_case("A")["real"][0]
    vis = attr > 5
    stream = dict(mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)
    calls = []

    def search(nq, k, seed):
        Q = sg.queries("A", nq, seed)
        dq = env.dev(Q)
        calls.append(("search (%d, %d)" % (nq, k), lambda o: ix.search(dq, k, out=tuple(o), **stream), lambda: env.outs(nq, k),
                      lambda: ix.search(Q, k, **stream), sg.topk_np(X, Q, k, vis)[:3]))

    def among(nq, k, shared, longest, seed):
        c = sg.among_case("A", nq, k, shared, seed=seed, longest=longest)
        Q, L = c["real"]
        dq, dl = env.dev(Q), env.dev(L)
        lists = L if shared else [L[c["offsets"][q]:c["offsets"][q + 1]] for q in range(nq)]
        calls.append((c["name"], lambda o: ix.search_among(dq, dl, k, offsets=c["offsets"], out=tuple(o)), lambda: env.outs(nq, k),
                      lambda: ix.search_among(Q, L, k, offsets=c["offsets"]), sg.topk_np(X, Q, k, sg.rows_mask(n, lists, nq) & vis[:, None])[:3]))

    search(4, 10, 31)
    among(4, 10, True, 300, 32)
    w = np.flatnonzero(vis)
    calls.append(("select (3, 50)", lambda o: ix.select(3, 50, out=tuple(o)), lambda: [env.full((50,), "int64"), env.full((2,), "int64")],
                  lambda: (lambda r: (r[0], np.array([len(r[0]), r[1]], np.int64)))(ix.select(3, 50)), (w[3:53].astype(np.int64), np.array([50, len(w)], np.int64))))
    search(64, 100, 33)            # run_buf_ and partial_buf_ regrow under pending work
    among(5, 10, False, 2000, 34)  # among_in_ regrows
    search(4, 10, 35)
    c = sg.range_case("A", seed=36)
    Q, radius = c["real"]
    dq = env.dev(Q)
    calls.append((c["name"], lambda o: ix.search_range(dq, radius, 16, flat_engine="stream", out=tuple(o)), lambda: env.outs(len(Q), 16, totals=True),
                  lambda: ix.search_range(Q, radius, 16, flat_engine="stream"), sg.topk_np(X, Q, 16, vis, radius=radius)))
    search(4, 10, 37)
    return calls, attr


def fresh_index(env, attr):
    """table A under the program filter, no scratch yet: run_buf_, partial_buf_ and among_in_ grow under the pending calls of the sequence"""
    ix = env.amd.GpuIndex(sg.SHAPES["A"][1], 0)
    ix.attach_rows(sg.table("A"))
    ix.set_filter_program(sg.SELECT_PROG, attr.reshape(-1, 1))
    return ix


@pytest.mark.parametrize("own", [False, True], ids=["the caller's stream", "the index's own stream"])
def test_b_back_to_back_calls_do_not_tread_on_each_other(env, own):
    """one index, one gate, no sync until the end; every call has its own outputs and must equal numpy and the same call made alone.  Then the
    same sequence behind set_stream(None): on the index's own stream, which torch cannot gate - issued without a sync, ended by ix.synchronize()."""
    s = env.s
    names = ("ids", "dist", "counts", "totals")
    attr = sg.select_case("A")["real"][0]
    ref_ix, ix = fresh_index(env, attr), fresh_index(env, attr)
    try:
        ref_calls, calls = back_to_back_calls(env, ref_ix)[0], back_to_back_calls(env, ix)[0]
        alone = []
        for name, _, _, host_call, want in ref_calls:
            r = host_call()
            ref_ix.synchronize()
            sg.same(r, want, "b alone: " + name, names)
            alone.append(r)
        ref_ix.set_stream(s.cuda_stream)
        env.sync()
        ms = sg.gate_for("b: eight calls back to back", lambda: [call(mk()) for _, call, mk, _, _ in ref_calls], s)
        outs = [mk() for _, _, mk, _, _ in calls]
        env.sync()
        ix.set_stream(None if own else s.cuda_stream)
        if not own:
            sg.gate(s, ms)
        for (_, call, _, _, _), o in zip(calls, outs):
            call(o)
        behind = sg.issued_behind(s)
        if own:
            ix.synchronize()
        else:
            s.synchronize()
        print("stream-order: b on %-24s all eight issued with the stream still busy: %s" % ("the index's own stream" if own else "the caller's stream", behind))
        for (name, _, _, _, want), o, a in zip(calls, outs, alone):
            got = [t.cpu().numpy() for t in o]
            tag = "b on %s, %s" % ("the index's own stream" if own else "the caller's stream", name)
            sg.same(got, want, tag + " - against numpy", names)
            sg.same(got, a, tag + " - against the same call made alone", names)
    finally:
        ref_ix.close()
        ix.close()


def test_b_set_stream_drains_the_stream_it_leaves(env):
    ix, s = env.index("A"), env.s
    out = [env.full((50,), "int64"), env.full((2,), "int64")]
    env.sync()
    ms = sg.gate_for("b: set_stream behind a select", lambda: ix.select(0, 50, out=tuple(out)), s)
    try:
        sg.gate(s, ms)
        ix.select(0, 50, out=tuple(out))
        assert sg.issued_behind(s), ASYNC_WHY % ("select", ms / 4, ms)
        ix.set_stream(None)
        assert s.query(), "set_stream returned with work of this index still pending on the stream it left"
        assert out[1].cpu().numpy().tolist() == [50, sg.SHAPES["A"][0]]
    finally:
        ix.set_stream(s.cuda_stream)


# ------------------------------------------------------------------------------------------------ c. borrowed device filters are read in place
@pytest.mark.parametrize("engine,nq", [("FLAT_STREAM", 8), ("FLAT_MFMA_I8", 300), ("FLAT_MFMA_I8", 8)])
@pytest.mark.parametrize("kind", ["deleted", "column"])
def test_c_borrowed_filters_are_read_in_place(env, kind, engine, nq):
    """installed ONCE; the buffer changes on the stream between two searches (nq = 8 under FLAT_MFMA_I8: the one-pass form where the library
    takes it).  An engine that keeps something derived from the buffer across calls answers the second search for the old contents."""
    torch, s, amd = env.torch, env.s, env.amd
    ix = env.index("B")
    case = sg.check_case(sg.filter_case("B", nq, 10, kind))
    name = "%s %s" % (case["name"], engine)
    kw = dict(mode=amd.MODE_FLAT, flat_engine=getattr(amd, engine))
    st1, st2 = (env.dev(a) for a in case["real"])
    buf = st1.clone()
    dq = env.dev(case["Q"])
    env.sync()
    try:
        if kind == "deleted":
            ix.set_deleted(buf)
        else:
            ix.set_int_filter(buf, "==", 0)

        def issue(o1=None, o2=None):
            with torch.cuda.stream(s):
                buf.copy_(st1)
                ix.search(dq, 10, out=tuple(o1 or env.outs(nq, 10)), **kw)
                buf.copy_(st2)
                ix.search(dq, 10, out=tuple(o2 or env.outs(nq, 10)), **kw)
                buf.copy_(st1)
        ms = sg.gate_for(name, issue, s)
        o1, o2 = env.outs(nq, 10), env.outs(nq, 10)
        with torch.cuda.stream(s):
            buf.copy_(st2)      # (before the gate: the state the FIRST search must not see)
        env.sync()
        sg.gate(s, ms)
        issue(o1, o2)
        behind = sg.issued_behind(s)
        s.synchronize()
        st = ix.stats()
        print("stream-order: %-58s returned behind the gate: %s  bits %d one_pass %d" % (name, behind, st["main_kernel_bits"], st["one_pass"]))
        g1, g2 = ([t.cpu().numpy() for t in o] for o in (o1, o2))
        sg.same(g1, case["want"], "%s: the FIRST search read %s state" % (name, "the second" if np.array_equal(g1[0], case["want_decoy"][0]) else "neither"), case["names"])
        sg.same(g2, case["want_decoy"], "%s: the SECOND search read %s state" % (name, "the first" if np.array_equal(g2[0], case["want"][0]) else "neither"), case["names"])
    finally:
        ix.set_deleted(None)
        ix.set_int_filter(None, None, 0)


# ------------------------------------------------------------------------------------------------ d. host arrays are consumed when the call returns
def host_cases(env):
    amd = env.amd
    stream = dict(mode=amd.MODE_FLAT, flat_engine=amd.FLAT_STREAM)

    def search(nq):
        c = sg.search_case("A", nq, 10, seed=41)
        return c, [0], lambda ix, h, dv, o: ix.search(h[0], 10, out=tuple(o), **stream), lambda: env.outs(nq, 10), c["want_decoy"]

    def among(shared):
        c = sg.among_case("A", 6, 10, shared, seed=42)
        off = c["offsets"]
        if shared:
            return c, [1], lambda ix, h, dv, o: ix.search_among(dv[0], h[0], 10, out=tuple(o)), lambda: env.outs(6, 10), c["want_decoy_list"]
        # the decoy offsets: the same lengths in reverse order (as long in all, no list longer than the longest real one)
        doff = np.concatenate([[0], np.cumsum(np.diff(off)[::-1])]).astype(np.int64)
        Ld = c["decoy"][1]
        want_decoy = sg.topk_np(sg.table("A"), c["real"][0], 10, sg.rows_mask(sg.SHAPES["A"][0], [Ld[doff[q]:doff[q + 1]] for q in range(6)], 6))[:3]
        c = dict(c, real=c["real"] + (off,), decoy=c["decoy"] + (doff,), want_decoy_host=want_decoy)
        return c, [1, 2], lambda ix, h, dv, o: ix.search_among(dv[0], h[0], 10, offsets=h[1], out=tuple(o)), lambda: env.outs(6, 10), want_decoy

    def radius():
        c = sg.range_case("A", seed=43)
        return c, [1], lambda ix, h, dv, o: ix.search_range(dv[0], h[0], 16, flat_engine="stream", out=tuple(o)), lambda: env.outs(4, 16, totals=True), c["want_decoy_radius"]
    return {"queries 255 KB": lambda: search(1020), "queries 300 KB": lambda: search(1200), "among one list": lambda: among(True),
            "among lists and offsets": lambda: among(False), "range radius": radius}


@pytest.mark.parametrize("which", ["queries 255 KB", "queries 300 KB", "among one list", "among lists and offsets", "range radius"])
@pytest.mark.parametrize("memory", ["page-locked", "pageable"])
def test_d_host_arrays_are_consumed_when_the_call_returns(env, memory, which):
    """device outputs, a gate in front, and straight after the call returns the host array is overwritten with the decoy FROM THE HOST: a copy that
    is still pending then (hipMemcpyAsync out of page-locked memory is truly asynchronous) takes the decoy, or a mix."""
    torch, s = env.torch, env.s
    ix = env.index("A")
    case, host_idx, call, make_outs, want_decoy = host_cases(env)[which]()
    name = "d %s, %s" % (which, memory)
    sg.check_case(case)
    real = [np.ascontiguousarray(case["real"][i]) for i in host_idx]
    decoy = [np.ascontiguousarray(case["decoy"][i]) for i in host_idx]
    host = [sg.pinned(a.shape, a.dtype) if memory == "page-locked" else np.empty_like(a) for a in real]
    dv = [env.dev(a) for i, a in enumerate(case["real"]) if i not in host_idx]
    env.sync()

    def issue(outs=None):
        for h, a in zip(host, real):
            h[...] = a
        call(ix, host, dv, outs or make_outs())
        for h, a in zip(host, decoy):      # the caller refills its buffer: the next batch
            h[...] = a
    ms = sg.gate_for(name, issue, s)
    outs = make_outs()
    env.sync()
    sg.gate(s, ms)
    for h, a in zip(host, real):
        h[...] = a
    call(ix, host, dv, outs)
    behind = sg.issued_behind(s)
    for h, a in zip(host, decoy):
        h[...] = a
    s.synchronize()
    got = [t.cpu().numpy() for t in outs]
    print("stream-order: %-58s returned behind the gate: %s; the answer is the %s input's" % (name, behind, sg.took(got[0], case["want"][0], want_decoy[0])))
    sg.same(got, case["want"], "%s: the host array was read AFTER the call returned - the answer is %s (by first ids)" % (
        name, {"decoy": "the decoy's", "a mix": "a mix of both", "neither": "neither's"}.get(sg.took(got[0], case["want"][0], want_decoy[0]), "?")), case["names"])


# ------------------------------------------------------------------------------------------------ e. the free functions with a stream= argument
def test_e_normalize_rows_on_a_stream(env):
    amd, s = env.amd, env.s
    case = sg.check_case(sg.normalize_case())
    alone, alone_decoy = ((amd.normalize_rows(case[which][0].copy(), only_if_nonzero=True),) for which in ("real", "decoy"))
    assert np.allclose(alone[0], case["want"][0], rtol=1e-6, atol=0)
    case = dict(case, want=alone, want_decoy=alone_decoy)      # (x / |x| in fp32: the bits are the library's own, made alone)
    windowed(env, case, lambda t, o: (amd.normalize_rows(t[0], only_if_nonzero=True, stream=s.cuda_stream), o[0].copy_(t[0])),
             lambda: [env.full(case["real"][0].shape, "float32")], alone=alone)


@pytest.mark.parametrize("packed", [False, True])
def test_e_merge_topk_on_a_stream(env, packed):
    amd, s, torch = env.amd, env.s, env.torch
    case = sg.merge_case("topk")
    G, nq, k = case["G"], case["nq"], case["k"]
    dist, ids = case["real"]
    alone = amd.merge_topk(dist, ids, np.empty((nq, k), F), np.empty((nq, k), np.int64))
    make_outs = lambda: [env.full((nq, k), "float32"), env.full((nq, k), "int64")]      # noqa: E731
    if not packed:
        windowed(env, case, lambda t, o: amd.merge_topk(t[0], t[1], o[0], o[1], stream=s.cuda_stream), make_outs, alone=alone)
        return
    # one gathered buffer: per shard [ids int64 [nq][k] | dist float32 [nq][k]]
    pack = lambda d, i: (np.concatenate([i.reshape(G, -1).view(np.uint8), d.reshape(G, -1).view(np.uint8)], axis=1),)      # noqa: E731
    case = dict(case, name=case["name"] + " packed", real=pack(*case["real"]), decoy=pack(*case["decoy"]))
    stride, off = nq * k * 12, nq * k * 8
    windowed(env, case, lambda t, o: amd.merge_topk_packed(t[0], stride, off, G, nq, k, o[0], o[1], stream=s.cuda_stream), make_outs, alone=alone)


def test_e_merge_range_on_a_stream(env):
    amd, s = env.amd, env.s
    case = sg.merge_case("range")
    nq, k = case["nq"], case["k"]
    alone = amd.merge_range(*case["real"])
    windowed(env, case, lambda t, o: amd.merge_range(*t, out=tuple(o), stream=s.cuda_stream), lambda: env.outs(nq, k, totals=True), alone=alone)


def test_e_merge_select_on_a_stream(env):
    amd, s = env.amd, env.s
    case = sg.merge_case("select")
    limit = case["k"] - 2      # (the case's window: skip 2, limit len - 2)
    w, total = amd.merge_select(*case["real"], skip=2, limit=limit)
    alone = (w, np.array([len(w), total], np.int64))
    windowed(env, case, lambda t, o: amd.merge_select(*t, skip=2, limit=limit, out=tuple(o), stream=s.cuda_stream),
             lambda: [env.full((limit,), "int64"), env.full((2,), "int64")], alone=alone)
