"""What a tiled context adds to determine_fractures (csrc/sz_fracture_tile.hpp), restated in numpy: the mean height of sz_k_frac_criterion --
1024 strided partial sums, each over its rows in ascending order, then the halving tree, divided by n -- over the heights gathered by global
number, and the alternative the library does NOT take: every rank reduces its own rows that way and the rank sums are added.  Also the one
field the one-pass GPU tests and the CPU test share."""
import numpy as np

TPB = 1024
ONE_PASS_N, ONE_PASS_SEED = 1500, 1500          # more floes than threads: a thread sums more than one row
# The heights are Uniform(0.1, 1.5) from a generator of their own.  The two orders of addition differ by an ulp of the sum at most, and
# the division by n hides that more often than not: of the seeds 1500 .. 1539 sixteen tell the orders apart for the 2-rank owners, ten for
# the 4-rank owners and six for both (wider ranges of magnitudes, log-uniform over 0.1 .. 9 or 0.01 .. 9, do no better: 10 and 7 of 60).
# 1502 is the first seed that does for both; tests/test_fracture_tiles_cpu.py asserts it.
ONE_PASS_HEIGHT_SEED = 1502


def kernel_sum(h):
    """sz_k_frac_criterion's sum of h: thread t takes rows t, t + 1024, .. ascending; then sh[t] += sh[t + w] for w = 512 .. 1"""
    h = np.asarray(h, np.float64)
    sh = np.zeros(TPB)
    for k in range(0, len(h), TPB):
        part = h[k:k + TPB]
        sh[:len(part)] += part
    w = TPB // 2
    while w > 0:
        sh[:w] += sh[w:2 * w]
        w //= 2
    return sh[0]


def kernel_mean(h):
    return kernel_sum(h) / float(len(h)) if len(h) else 0.0


def gathered_mean(h, owner, nranks):
    """the library's way: every rank packs {global number, height} of its rows, the records are gathered, each height goes to its global
    number, the kernel runs over that array"""
    owner = np.asarray(owner)
    out = np.full(len(h), np.nan); mark = np.zeros(len(h), int)
    for r in range(nranks):
        g = np.nonzero(owner == r)[0]
        out[g] = np.asarray(h)[g]; mark[g] += 1
    assert np.all(mark == 1)
    return kernel_mean(out)


def reduced_mean(h, owner, nranks):
    """the wrong alternative: per-rank kernel sums, added in rank order"""
    owner = np.asarray(owner)
    s = 0.0
    for r in range(nranks):
        s += kernel_sum(np.asarray(h)[owner == r])
    return s / float(len(h))


def one_pass_case():
    """(cfg, stress_accum, area, height): the configs[1]-style field of 1 500 floes -- its centroids give the ranks' rows, interleaved in
    global order under tiles.assign_tiles -- and random symmetric stress_accum, heights and areas in the manner of
    test_fracture_gpu.py::_random_world (a fifth of the areas under min_floe_area = 1e6)"""
    from subzero_jl_amd import fields
    n = ONE_PASS_N
    cfg = fields.make_config(n_floes=n, seed=91)
    assert cfg["n_floes"] == n == len(cfg["derived"]["cx"])
    rng = np.random.default_rng(ONE_PASS_SEED)
    area = np.where(rng.random(n) < 0.2, rng.uniform(1e4, 1e6, n), rng.uniform(1e6, 1e9, n))
    height = np.random.default_rng(ONE_PASS_HEIGHT_SEED).uniform(0.1, 1.5, n)
    s11, s22, s12 = rng.normal(0, 6e4, n) - 2e4, rng.normal(0, 6e4, n) - 2e4, rng.normal(0, 3e4, n)
    return cfg, np.stack([s11, s12, s12, s22], 1), area, height


def one_pass_owners(cfg, nranks):
    from subzero_jl_amd import tiles
    return tiles.assign_tiles(cfg["derived"]["cx"], cfg["derived"]["cy"], cfg["L"], nranks)
