"""A Python replay of the dense-tail plan's item rule with the per-tile-pair reach (csrc/plan.hip: plan_dense_level and
emit_dense_items, single device, look-ahead on), from the arrays of the host analysis alone -- nothing here calls the device.

For every tail front jj: its active descendants (`tail_blk`: the tail fronts whose true rows reach jj's columns), the tile pairs
a descendant reaches at all (`pair_on`), the K segments of the late (last `depth` descendants) and the early launch, and per item
(tile pair, segment) the trim of the segment to the first and last descendant that reaches the pair's 256 rows.  `replay()` returns
what the plan reports: kept and all (tile pair, descendant) products, empty items, early and late items.
"""
import bisect

import numpy as np

TM = 128


def _active_runs(src, lo, hi):
    runs = []
    for d in src[bisect.bisect_left(src, lo):]:
        if d >= hi:
            break
        if runs and runs[-1][1] == d:
            runs[-1][1] = d + 1
        else:
            runs.append([d, d + 1])
    if len(runs) > 16:
        runs = [[runs[0][0], runs[-1][1]]]
    return runs


def _cut_runs(runs, total, nseg):
    out = []
    for first, end in runs:
        ln = end - first
        ns_r = max(1, min(ln, (nseg * ln + total // 2) // total))
        for q in range(ns_r):
            a, b = first + ln * q // ns_r, first + ln * (q + 1) // ns_r
            if b > a:
                out.append((a, b))
    return out


def _segments(src, lo, hi, np_on, dense_items, dense_fill, taper):
    runs = _active_runs(src, lo, hi) if hi > lo else []
    total = sum(b - a for a, b in runs)
    if total == 0:
        return []
    want = max(1, (dense_items + max(1, np_on) // 2) // max(1, np_on))
    cap = min(64, total)
    nseg = min(cap, want)
    if dense_fill and np_on > 0:
        best = -1.0
        for ns in range(max(1, want * 2 // 3), min(cap, want * 3 // 2 + 1) + 1):
            items = np_on * len(_cut_runs(runs, total, ns))
            rounds = (items + dense_fill - 1) // dense_fill
            score = items / float(rounds * dense_fill) - 0.02 * abs(ns - want) / float(want)
            if score > best:
                best, nseg = score, ns
    out = _cut_runs(runs, total, nseg)
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


def replay(sym, dense_items=128, dense_fill=256, depth=2):
    """dict(all, kept, empty, early, late) of the handle's dense-tail plan (dense_items >= 64 as the plan clamps it)."""
    info = sym.info()
    start = sym.get("sn_start").astype(np.int64)
    tile_base = sym.get("tile_base").astype(np.int64)
    bptr = sym.get("tail_blk_ptr").astype(np.int64)
    blk = sym.get("tail_blk").astype(np.int64)
    df, ns, n = info.dense_first, info.nsuper, info.n
    nT = ns - df
    known = bptr.size > 0                              # (no block pattern: every descendant counts as reaching everything)
    tail_src = [[] if known else list(range(nT)) for _ in range(nT)]
    for d in range(nT if known else 0):
        for f in blk[bptr[d]:bptr[d + 1]]:
            tail_src[int(f)].append(d)
    c0t = int(start[df])
    col_front = np.searchsorted(start[df:ns + 1], np.arange(c0t, n), side="right") - 1
    dense_items = max(64, dense_items)
    taper = dense_items >= 1024
    res = dict(all=0, kept=0, empty=0, early=0, late=0)
    for jj in range(nT):
        fr = df + jj
        ntl = int(tile_base[fr + 1] - tile_base[fr])
        npairs = (ntl + 1) // 2
        src = tail_src[jj]
        act = set(src[:bisect.bisect_left(src, jj)])
        c0j = int(start[fr])
        fronts = []                                    # per pair: None (the target's own columns) or (f_lo, f_hi)
        pair_on = []
        for pq in range(npairs):
            lo = c0j + 2 * TM * pq
            hi = min(lo + 2 * TM, n)
            f_lo, f_hi = int(col_front[lo - c0t]), int(col_front[hi - 1 - c0t])
            if f_lo <= jj:
                fronts.append(None)
                pair_on.append(True)
                continue
            fronts.append((f_lo, f_hi))
            pair_on.append(jj == 0 or any(act.intersection(tail_src[f]) for f in range(f_lo, f_hi + 1)))
        np_on = sum(pair_on)
        dcnt_l = min(depth, jj)
        segs_l = _segments(src, jj - dcnt_l, jj, np_on, dense_items, dense_fill, False)
        segs_e = _segments(src, 0, jj - dcnt_l, np_on, dense_items, dense_fill, taper)
        for which, segs in (("early", segs_e), ("late", segs_l)):
            for k0, k1 in segs:
                for pq in range(npairs):
                    if not pair_on[pq]:
                        continue
                    res[which] += 1
                    res["all"] += k1 - k0
                    a, b = k0, k1
                    if fronts[pq] is not None and jj > 0:
                        first, last = k1, k0 - 1
                        for f in range(fronts[pq][0], fronts[pq][1] + 1):
                            sf = tail_src[f]
                            x, y = bisect.bisect_left(sf, k0), bisect.bisect_left(sf, k1)
                            if x != y:
                                first, last = min(first, sf[x]), max(last, sf[y - 1])
                        a, b = (k0, k0) if first > last else (first, last + 1)
                    res["kept"] += b - a
                    res["empty"] += b <= a
    return res
