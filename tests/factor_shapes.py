"""The problems of tests/test_gpu_factor_schedules.py, the facts of the host analysis its cases rely on, and a Python replay
of the K-segment rule of the dense-tail plan (host only; nothing here calls the device).

The four dense problems are V = G G^T + n I with G an n x 64 standard normal matrix (seed 0) in the natural order: every
front is a tail front, so `max_width` alone decides the width of the fronts, the depth of the B chunks a descendant is
streamed in (64 columns per chunk) and the width of the last, ragged front.  cond(V) < 2, so the oracle's factor is good to
about 1e-14.  The two pedigrees are those of test_gpu_parity's schedule tests: a prelude under a padded tail (P10), and the
tail that is moved to the end of the order (P20).

`tests/test_factor_shapes.py` asserts FACTS[...] without a GPU; a change of the ordering or of the tail selection fails there
instead of quietly moving the GPU cases off the kernels' edges.
"""
import numpy as np
import scipy.sparse as sp

TM = 128      # rows of a tile (csrc: TM); a dense item takes a pair of tiles
LOOK_DEPTH = 2


def dense_lowrank_spd(n, k=64, seed=0):
    G = np.random.default_rng(seed).standard_normal((n, k))
    return sp.csr_matrix(G @ G.T + n * np.eye(n))


def _dense_problem(n, **opts):
    return dict(mats=[dense_lowrank_spd(n)], sigma2=[1.0], opts=dict(ordering="natural", **opts))


def _pedigree_problem(n0, seed):
    from tests.helpers import small_pedigree
    A, _ = small_pedigree(n0, 0.01, seed)
    return dict(mats=[A, sp.identity(A.shape[0], format="csr")], sigma2=[0.35, 0.65], opts={})


# id -> (builder, facts of the host analysis)
#   tail: widths of the tail fronts; outside: prelude fronts that reach the tail, groups of identical tail rows, groups with
#   2 or more members, block pairs (128 x 128 blocks of the lower triangle of the leaders' tail rows)
PROBLEMS = {
    "R37": (lambda: _dense_problem(3000, max_width=37), dict(n=3000, nsuper=82, dense_first=0, tail=[37] * 81 + [3])),
    "R50": (lambda: _dense_problem(700, max_width=50), dict(n=700, nsuper=14, dense_first=0, tail=[50] * 14)),
    "R100": (lambda: _dense_problem(700, max_width=100), dict(n=700, nsuper=7, dense_first=0, tail=[100] * 7)),
    "R128": (lambda: _dense_problem(5000), dict(n=5000, nsuper=40, dense_first=0, tail=[128] * 39 + [8])),
    "P10": (lambda: _pedigree_problem(10000, 5),
            dict(n=8128, nsuper=1154, dense_first=1144, tail=[89] + [128] * 8 + [31],
                 outside=dict(descendants=412, groups=381, multi=29, pairs=503))),
    "P20": (lambda: _pedigree_problem(20000, 1),
            dict(nsuper_tail=24, tail_columns=2957, first_width=45, outside=dict(descendants=950, groups=915))),
}
_BUILT = {}


def problem(pid):
    """The problem's matrices, sigma2 and Symbolic options; built once."""
    if pid not in _BUILT:
        _BUILT[pid] = PROBLEMS[pid][0]()
    return _BUILT[pid]


def release():
    _BUILT.clear()


def tail_pairs(sym):
    """Per tail front: tile pairs of the front (two vertically adjacent 128-row tiles are one dense item's rows)."""
    info = sym.info()
    tb = sym.get("tile_base").astype(np.int64)
    ntl = np.diff(tb)[info.dense_first:info.nsuper]
    return (ntl + 1) // 2


def single_descendant_early_items(sym, depth=LOOK_DEPTH):
    """Early dense items of a plan whose every K segment is ONE descendant long: sum over the tail fronts of
    (tile pairs) x (jj - depth).  (Every tile pair counts: exact on a dense matrix, an upper bound where the plan skips the
    tile pairs that only padding reaches.)"""
    np_on = tail_pairs(sym)
    jj = np.arange(np_on.size)
    return int((np_on * np.maximum(jj - depth, 0)).sum())


def outside_groups(sym):
    """The prelude fronts k_outside serves (finished below the tail's first level, with rows among the tail's columns), the
    groups of identical tail rows among them and the block pairs of the group leaders: plan_outside's rule in numpy."""
    info = sym.info()
    start = sym.get("sn_start").astype(np.int64)
    rowptr = sym.get("sn_rowptr").astype(np.int64)
    rows = sym.get("sn_rows")
    level = sym.get("sn_level")
    c0 = start[info.dense_first]
    tail_level = level[info.dense_first]
    groups = {}
    for d in range(info.dense_first):
        if level[d] >= tail_level:
            continue
        r = rows[rowptr[d]:rowptr[d + 1]]
        t = r[np.searchsorted(r, c0):]
        if t.size:
            groups.setdefault(t.tobytes(), []).append(d)
    sizes = [len(v) for v in groups.values()]
    per_panel = {}                                 # first tail panel -> block-pair items that start there
    for key in groups:
        t = np.frombuffer(key, dtype=rows.dtype)
        nb = (t.size + TM - 1) // TM
        for bj in range(nb):                       # an item's first panel is the panel of the first row of its block bj
            f = int(np.searchsorted(start, t[TM * bj], side="right") - 1)
            per_panel[f] = per_panel.get(f, 0) + nb - bj   # (bi = bj .. nb - 1)
    return dict(descendants=int(sum(sizes)), groups=len(sizes), multi=sum(1 for s in sizes if s > 1),
                pairs=int(sum(per_panel.values())), first_panels=len(per_panel), max_members=max(sizes),
                per_panel=[per_panel[f] for f in sorted(per_panel)])


def outside_chunks(per_panel, want):
    """Launches of k_outside for `want` requested chunks: the items are sorted by first panel and cut about every
    ceil(N / want) items, at the next change of the first panel; `want` >= the number of first panels: one chunk per panel."""
    N, want = int(sum(per_panel)), max(1, int(want))
    per = 1 if want >= len(per_panel) else max(1, (N + want - 1) // want)
    ends = np.cumsum(per_panel)
    nch, i = 0, 0
    while i < N:
        i = int(ends[np.searchsorted(ends, min(N, i + per))])
        nch += 1
    return nch


# ---- the K-segment rule of the dense-tail plan (csrc/plan.hip, plan_dense_level), one active run per target

def _cut_run(total, nseg):
    """cut_runs on one run of `total` descendants: its segments as (first, end) pairs."""
    ns = max(1, min(total, (nseg * total + total // 2) // total))
    out = []
    for q in range(ns):
        a, b = total * q // ns, total * (q + 1) // ns
        if b > a:
            out.append((a, b))
    return out


def k_segments(total, np_on, dense_items, dense_fill=256, taper=False):
    """The K segments of `total` consecutive descendants of a target with `np_on` tile pairs."""
    if total <= 0:
        return []
    want = max(1, (dense_items + max(1, np_on) // 2) // max(1, np_on))
    cap = min(64, total)
    nseg = min(cap, want)
    if dense_fill and np_on > 0:
        best = -1.0
        for ns in range(max(1, want * 2 // 3), min(cap, want * 3 // 2 + 1) + 1):
            items = np_on * len(_cut_run(total, ns))
            rounds = (items + dense_fill - 1) // dense_fill
            score = items / float(rounds * dense_fill) - 0.02 * abs(ns - want) / float(want)
            if score > best:
                best, nseg = score, ns
    out = _cut_run(total, nseg)
    if taper and len(out) >= 3:
        tp = out[:-2]
        for (a0, b0), parts in ((out[-2], 2), (out[-1], 4)):
            ln = b0 - a0
            for q in range(parts):
                a, b = a0 + ln * q // parts, a0 + ln * (q + 1) // parts
                if b > a:
                    tp.append((a, b))
        out = tp
    return out


def replay_early_items(np_on, dense_items, dense_fill=256, taper=False, depth=LOOK_DEPTH):
    """(early items, longest early segment in descendants) of a dense matrix's plan: target jj takes its descendants
    0 .. jj - depth - 1 early, every tile pair on."""
    items, longest = 0, 0
    for jj, npj in enumerate(np_on):
        segs = k_segments(jj - min(depth, jj), int(npj), max(64, dense_items), dense_fill, taper)
        items += int(npj) * len(segs)
        longest = max([longest] + [b - a for a, b in segs])
    return items, longest
