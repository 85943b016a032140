"""What the half scan's walk (csrc/half.hip: half_scan_kernel) is held to once a slice is longer than one round of 64 rows, in numpy: the plan of
csrc/half_host.hpp restated, and a model that says, from a table's distances alone, which rounds take the hit path.

  plan(n, dim, nq, k)    half_plan and half_seed_rows restated from their comments and constants, not imported: nb, kpl, cols, tiles, slices,
                         rows_per_slice, rounds, and seed_rows with the prefix's own plan under "seed" (None: the call is not seeded).
  walk(D, ...)           one launch.  D [rows][distinct queries] are fp64 distances that are fp32 numbers (exact_ref.dist64 on a table fp32 computes
                         exactly), so a distance's ordinal - make_key's high word - is known without a device.  Slice s walks rows
                         [s * rows_per_slice, ...) in rounds of 64 STORED rows: deleted rows and the zero rows behind n in the last round are
                         stored and vote, rows past the padded table are not.  Round r of slice s of a tile is a hit iff for some query q of the
                         tile and some of its 64 rows  !(d >= T_q),  T_q exclusive:
                           bound_q = min(k-th ordinal of the slice's list before round r, the launch's opening bound of q);  open: 0xFFFFFFFF
                           vote    = d is a NaN, or ordinal(d) < bound_q     (a bound above +inf's ordinal is a NaN threshold: everything passes)
                         The list of (slice, q) holds the k smallest (ordinal, row) among the rows of the rounds before that are visible and
                         under the opening bound: rows ascend, so the kernel's one-by-one strict compare against the k-th ordinal keeps exactly
                         those.  Columns a tile does not have carry -inf and vote only on a NaN, which a row with a NaN element gives its live
                         columns too; the model needs no rule for them.
  search(D, ...)         a call: the seed launch over the prefix (the same walk, started open), seed = the ordinal of the prefix's k-th visible
                         distance + 1 or open, the main launch from it, the slices' lists merged.

The batch is given as `qmap`: query q of the batch is column qmap[q] of D, so a long batch of few distinct queries costs the few.
tests/test_half_walk_ref_cpu.py holds the merged lists to np.lexsort and the plan to literals; tests/test_gpu_half_rounds.py holds the device's
hit_rounds and seed_hit_rounds to these numbers.  Integers only past the distances; nothing here is fitted to device output."""
import numpy as np

from merge_ref import ORD_NAN, ord2f, ordinal

OPEN = 0xFFFFFFFF
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
WAVE_ROWS, BLOCK_WAVES, LIST_BUDGET, LDS_QUERY_BYTES, MAX_BLOCKS, MERGE_KEYS, SEED_MIN_ROWS = 64, 4, 64, 131072, 2048, 1 << 18, 32768
_NEVER = np.int64(1) << 40   # a row that is not stored: no bound lets it vote

# The shapes at which a slice walks more than one round (tests/native/half_host_check.cpp pins the same numbers to half_plan itself):
# tag: (n, dim, nq, k), (cols, kpl, nb), tiles, (slices, rows_per_slice), seed_rows, (seed slices, seed rows_per_slice)
SHAPES = {
    "R1": ((32767, 40, 2053, 10), (64, 1, 4), 33, (248, 192), 0, None),
    "R1s": ((40000, 40, 2053, 10), (64, 1, 4), 33, (248, 192), 4096, (64, 64)),
    "R2": ((60000, 40, 5, 1024), (4, 16, 1), 2, (256, 256), 8192, (128, 64)),
    "R3": ((40000, 40, 300, 1024), (4, 16, 1), 75, (108, 384), 8192, (108, 128)),
    "R4": ((15000, 40, 2060, 129), (16, 4, 1), 129, (60, 256), 0, None),
    "R5": ((24000, 40, 2060, 65), (32, 2, 2), 65, (124, 256), 0, None),
    "R6": ((24000, 1056, 2060, 10), (32, 1, 2), 65, (124, 256), 0, None),
    "R7": ((15000, 2080, 2060, 10), (16, 1, 1), 129, (60, 256), 0, None),
    "R8": ((12000, 40, 2060, 257), (8, 8, 1), 258, (28, 448), 0, None),
}


def seed_rows(n, k):
    """a sixteenth of the table, at least 4096 rows and 8 k, in whole passes of 256 rows; no seed below 32768 rows"""
    if n < SEED_MIN_ROWS:
        return 0
    return (max(n // 16, 4096, 8 * k) + 255) // 256 * 256


def _launch_plan(n, dim, nq, k):
    d_pad = (dim + 31) // 32 * 32
    kpl = 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16
    nb = 4
    while nb > 1 and (16 * nb > LIST_BUDGET // kpl or nb * 32 * d_pad > LDS_QUERY_BYTES or nq <= 16 * (nb // 2)):
        nb //= 2
    cols = min(LIST_BUDGET // kpl, 16 * nb)
    tiles = -(-nq // cols)
    gx = -(-n // (WAVE_ROWS * BLOCK_WAVES))
    gx = max(1, min(gx, MAX_BLOCKS // max(tiles, 1), MERGE_KEYS // (k * BLOCK_WAVES)))
    slices = gx * BLOCK_WAVES
    rps = max(WAVE_ROWS, -(-(-(-n // slices)) // WAVE_ROWS) * WAVE_ROWS)
    return dict(nb=nb, kpl=kpl, cols=cols, tiles=tiles, slices=slices, rows_per_slice=rps, rounds=-(-n // WAVE_ROWS) * tiles)


def plan(n, dim, nq, k):
    p = _launch_plan(n, dim, nq, k)
    p["seed_rows"] = seed_rows(n, k)
    p["seed"] = _launch_plan(p["seed_rows"], dim, nq, k) if p["seed_rows"] else None
    return p


def walk(D, visible, pl, k, qmap, pad=None, opening=None):
    """One launch over the rows of D [n][U] under plan `pl` (slices, rows_per_slice, cols).  visible: bool [n] or None; qmap: int [nq], the column
    of D each query of the batch is; pad [U]: the distance of a zero row (needed when n is not whole rounds); opening [U]: the bound every slice
    starts from (None: open).  Returns (hit rounds, keys [U][k] uint64 of the merged lists: ordinal << 32 | row, EMPTY behind the last)."""
    n, U = D.shape
    S, rps, cols = pl["slices"], pl["rows_per_slice"], pl["cols"]
    R, P, n_pad = rps // WAVE_ROWS, S * rps, -(-n // WAVE_ROWS) * WAVE_ROWS
    assert P >= n and rps % WAVE_ROWS == 0
    o = ordinal(np.ascontiguousarray(D.T)).astype(np.int64)                     # [U][n]
    opening = np.full(U, OPEN, np.int64) if opening is None else np.asarray(opening, np.int64)
    stored = np.full((U, P), _NEVER, np.int64)
    stored[:, :n] = o
    if n_pad > n:
        stored[:, n:n_pad] = ordinal(pad).astype(np.int64)[:, None]
    enters = (o < opening[:, None]) & (True if visible is None else np.asarray(visible, bool)[None, :])
    key = np.full((U, P), EMPTY, np.uint64)
    key[:, :n] = np.where(enters, (o.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :], EMPTY)
    key = key.reshape(U, S, rps)
    bound = np.full((U, S, R), OPEN, np.int64)
    for r in range(1, R):
        if r * WAVE_ROWS >= k:                                                   # the list before round r: its k-th entry, or none yet
            bound[:, :, r] = (np.partition(key[:, :, :r * WAVE_ROWS], k - 1, axis=2)[:, :, k - 1] >> np.uint64(32)).astype(np.int64)
    bound = np.minimum(bound, opening[:, None, None])
    stored = stored.reshape(U, S, R, WAVE_ROWS)
    vote = ((stored < bound[..., None]) | (stored == int(ORD_NAN))).any(3)       # [U][S][R]
    walked = (np.arange(S)[:, None] * rps + np.arange(R)[None, :] * WAVE_ROWS) < n
    qmap = np.asarray(qmap)
    hits = sum(int((vote[np.unique(qmap[q0:q0 + cols])].any(0) & walked).sum()) for q0 in range(0, len(qmap), cols))
    lists = np.sort(key, axis=2)[:, :, :k]                                      # what each wavefront stores: partial[q][slice][k]
    merged = np.sort(lists.reshape(U, -1), axis=1)[:, :k]
    if merged.shape[1] < k:
        merged = np.concatenate([merged, np.full((U, k - merged.shape[1]), EMPTY, np.uint64)], axis=1)
    return hits, merged


def search(D, visible, dim, k, qmap, pad=None):
    """A call of eps_half_index_search on a table whose distances to the distinct queries are D [n][U].  Returns a dict: plan, hit_rounds,
    seed_hit_rounds, seed [U] (the opening bounds of the main launch; None if not seeded), rows [U][k] (-1 behind the last), dist [U][k] float32,
    counts [U]"""
    n, U = D.shape
    pl = plan(n, dim, len(qmap), k)
    seed_hits, opening = 0, None
    if pl["seed_rows"]:
        sr = pl["seed_rows"]
        seed_hits, top = walk(D[:sr], None if visible is None else np.asarray(visible, bool)[:sr], pl["seed"], k, qmap)
        kth = top[:, k - 1]
        opening = np.where(kth == EMPTY, OPEN, (kth >> np.uint64(32)).astype(np.int64) + 1)
    hits, top = walk(D, visible, pl, k, qmap, pad, opening)
    found = top != EMPTY
    return dict(plan=pl, hit_rounds=hits, seed_hit_rounds=seed_hits, seed=opening, counts=found.sum(1),
                rows=np.where(found, (top & np.uint64(0xFFFFFFFF)).astype(np.int64), -1),
                dist=np.where(found, ord2f((top >> np.uint64(32)).astype(np.uint32)), np.float32(np.inf)).astype(np.float32))
