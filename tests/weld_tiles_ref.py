"""The partition rule of the tiled welding pass (csrc/sz_weld_tile.hpp, DESIGN.md §9c "tiled contexts") restated in numpy over the global
columns and an ownership vector: what each rank computes from the gathered candidate records alone.  Numbers are 0-based global floe numbers."""
import numpy as np

ACTIVE = 1


def verdict(cx, cy, rmax, a, b):
    """potential_interaction with floe a in the place of the floe with the smaller number (strict <, parents only)"""
    ddx, ddy, rr = cx[a] - cx[b], cy[a] - cy[b], rmax[a] + rmax[b]
    return (ddx * ddx + ddy * ddy) < rr * rr


def break_number(in_bounds, owner, nranks):
    """the number bin_floe_centroids breaks at: every rank's smallest owned number with an out-of-bounds centroid, then the minimum over the
    ranks (n: none)"""
    n = len(in_bounds)
    per_rank = [min((g for g in np.nonzero(owner == r)[0] if not in_bounds[g]), default=n) for r in range(nranks)]
    return min(per_rank), per_rank


def rank_work(r, owner, bin_, cx, cy, rmax, area, status, max_weld_area, n):
    """what rank r finds in its walk: the keys (k n + i) n + j of the pairs it owns (i owned, j > i anywhere), ascending, and the set of its
    owned floes that are wanted (a partner with a smaller number lives on another rank)"""
    ok = (bin_ >= 0) & (status == ACTIVE) & (area < max_weld_area)
    keys, wanted = [], set()
    for i in np.nonzero(ok & (owner == r))[0]:
        for j in np.nonzero(ok & (bin_ == bin_[i]))[0]:
            if j == i:
                continue
            lo, hi = (i, j) if i < j else (j, i)
            if not verdict(cx, cy, rmax, lo, hi):
                continue
            if j > i:
                keys.append((int(bin_[i]) * n + int(i)) * n + int(j))
            elif owner[j] != r:
                wanted.add(int(i))
    return sorted(keys), wanted


def merge(per_rank_keys, n):
    """the ranks' ascending, disjoint key lists into one ascending list of (k, i, j)"""
    allk = sorted(k for ks in per_rank_keys for k in ks)
    return [(k // (n * n), (k // n) % n, k % n) for k in allk]
