"""The frame dispatch plan (csrc/rt_dispatch.h plan_frame, through rt_debug_frame_plan) on the CPU: which kernel
renders a frame, whether it needs the variants library, its block order, longest-first eligibility and wave split,
over the full product of modes x depths x flags x alone x shards x scene sizes x frame sizes x kernel variants. The
expected values are written out here from the documented rules (rt_api.h rt_frame / rt_debug_set_variant /
rt_debug_frame_plan), as numpy columns over all cases; never taken from a second call of the hook."""
from types import SimpleNamespace

import numpy as np
import pytest

from kernel_variants import LPT_IN_FLIGHT, NO_LPT, VARIANTS, VARIANTS_LIB

PRIMARY, FULL, BOX = 0, 1, 2
STATS, TIMELINE, WAVE_STATS = 2, 4, 8
NONE, GENERIC, FUSED, TRACE_SHADE, DUAL, TWO_RAYS, PERSISTENT, MEGAKERNEL, PIPELINE = range(9)
L2_BYTES = 32 << 20  # 8 XCDs x 4 MiB: scenes whose records fit are "small"
SMALL, LARGE = 5 << 20, 150 << 20  # record bytes of a bunny-sized and a soup-sized scene
SIZES = [(16, 16), (24, 16), (640, 360), (1920, 1080)]
PRODUCT_BITS = [0] + sorted(VARIANTS.values()) + [NO_LPT, LPT_IN_FLIGHT]
LIB_BITS = sorted(VARIANTS_LIB.values())
IN = ("mode", "max_depth", "flags", "tiles_x", "tiles_y", "shard_index", "shards", "bits", "bytes", "wide4", "alone")
OUT = ("kernel", "trav", "needs_variants", "grid", "units", "depth", "l2_resident", "xcd_remap", "writes_wave_stats",
       "lpt", "split_ceiling", "rotate_bands", "pipeline_buffers", "full_small_build")


@pytest.fixture(scope="module")
def c(rt):
    """Every enumerated case once, inputs and plan as int64 columns (c.mode, c.kernel, ...), plus the derived columns
    the rules below share."""
    fn = rt.lib().rt_debug_frame_plan
    axes = ((PRIMARY, FULL, BOX), range(6), (0, STATS, STATS | WAVE_STATS, WAVE_STATS), range(len(SIZES)), (1, 8),
            PRODUCT_BITS + LIB_BITS, (SMALL, LARGE), (0, 1), (1, 0))
    m, d, f, size, sh, b, nb, w4, al = (a.reshape(-1) for a in np.meshgrid(*(np.array(a, np.int64) for a in axes), indexing="ij"))
    tiles = np.array([((W + 15) // 16, (H + 15) // 16) for W, H in SIZES], np.int64)[size]
    inp = np.ascontiguousarray(np.stack([m, d, f, tiles[:, 0], tiles[:, 1], 0 * m, sh, b, nb, w4, al], axis=1))
    out = np.zeros((len(inp), len(OUT)), np.int32)
    pin, pout, rc = inp.ctypes.data, out.ctypes.data, 0
    for i in range(len(inp)):
        rc |= fn(pin + 88 * i, 11, pout + 56 * i, 14)
    assert rc == 0
    c = SimpleNamespace(n=len(inp), **dict(zip(IN, inp.T)), **dict(zip(OUT, out.T.astype(np.int64))))
    c.stats = (c.flags & STATS) != 0
    c.prim = c.mode != FULL  # PRIMARY or box colours: the PRIMARY kernels' dispatch
    c.own_depth = np.where(c.mode == FULL, 2, 1)
    # rt_api.h rt_frame.max_depth: the tuned kernels at the mode's own depth, the generic kernel at any other (or
    # under variant 65536); box colours have one depth and one kernel
    c.generic = (c.mode != BOX) & (((c.max_depth > 0) & (c.max_depth != c.own_depth)) | ((c.bits & 65536) != 0))
    c.dual = (c.prim & ~c.stats & ((c.max_depth <= 1) | (c.mode == BOX)) & ((c.bits & 1048576) != 0) &
              ((c.bits & (1 | 2 | 4 | 256 | 2048 | 32768 | 65536)) == 0))
    c.lds = ((c.bits & 1) == 0) & ~(((c.bits & 2) != 0) & (c.wide4 != 0))
    c.small = c.bytes <= L2_BYTES
    # rt_api.h rt_frame: a split frame's 16x16 tiles go by 4x4-tile super-tiles, super-tile s to shard s % count, and
    # every shard enumerates whole super-tiles (shard 0 here); an unsplit frame has its tiles
    n_super = ((c.tiles_x + 3) // 4) * ((c.tiles_y + 3) // 4)
    c.slots = np.where(c.shards == 1, c.tiles_x * c.tiles_y, 16 * ((n_super + c.shards - 1) // c.shards))
    return c


def check(c, ok, what):
    bad = np.flatnonzero(~np.asarray(ok, bool))
    if len(bad):
        i = bad[0]
        row = {k: int(getattr(c, k)[i]) for k in IN + OUT}
        pytest.fail(f"{what}: {len(bad)} of {c.n} cases, first {row}")


def test_rejects_bad_arguments(rt):
    with pytest.raises(rt.RTError):
        rt.frame_plan(PRIMARY, 0, 0, 0, 1, 0, 1, 0, SMALL, False, True)  # no tiles
    with pytest.raises(rt.RTError):
        rt.frame_plan(PRIMARY, 0, 0, 1, 1, 8, 8, 0, SMALL, False, True)  # shard 8 of 8
    p = rt.frame_plan(FULL, 0, 0, 120, 68, 0, 1, 0, SMALL, False, True)
    assert list(p) == list(OUT) and p["kernel"] == MEGAKERNEL and p["depth"] == 2 and p["l2_resident"] == 1


def test_product_bits_never_need_the_variants_library(c):
    assert c.n == 3 * 6 * 4 * 4 * 2 * 21 * 2 * 2 * 2
    check(c, ~np.isin(c.bits, PRODUCT_BITS) | (c.needs_variants == 0), "a product bit needs the variants library")


def test_variants_library_bits_need_it(c):
    """CPU twin of test_product_library_refuses_variant_only_kernels: without stats, bit 16 for FULL; 256, 2048 and
    1048576 for PRIMARY; bit 1 for every frame; bit 2 only when the scene has the quantised tree."""
    sel = np.isin(c.bits, LIB_BITS) & ~c.stats
    want = (~c.lds | c.dual | ((c.mode == FULL) & ((c.bits & 16) != 0)) | (c.prim & ((c.bits & (256 | 2048)) != 0)))
    check(c, ~sel | (c.needs_variants == want), "needs_variants")
    # the GPU test's frames, spelt out per named variant
    for mode, needing in ((PRIMARY, {1, 256, 2048, 2048 | 4096, 1048576}), (FULL, {1, 16, 48, 240})):
        for bits in LIB_BITS:
            rows = sel & (c.mode == mode) & (c.max_depth == 0) & (c.bits == bits)
            expect = (c.wide4 != 0) if bits == 2 else np.full(c.n, bits in needing)
            check(c, ~rows | (c.needs_variants == expect), f"needs_variants, mode {mode} variant {bits}")


def test_kernel_chosen(c):
    check(c, (c.grid == c.slots) & (c.grid > 0), "grid")
    check(c, c.trav == np.where((c.bits & 1) != 0, 0, np.where(c.lds, 1, 2)), "trav")
    check(c, c.depth == np.where((c.max_depth > 0) & (c.mode != BOX), c.max_depth, c.own_depth), "depth")
    # the default build, as rt_api.h documents it
    v0 = c.bits == 0
    d = c.max_depth
    table = [(c.mode == PRIMARY) & ~c.stats & (d <= 1), FUSED], [(c.mode == PRIMARY) & (d >= 2), GENERIC], \
            [(c.mode == PRIMARY) & c.stats & (d <= 1), TRACE_SHADE], [(c.mode == FULL) & np.isin(d, (0, 2)), MEGAKERNEL], \
            [(c.mode == FULL) & np.isin(d, (1, 3, 4, 5)), GENERIC], [(c.mode == BOX) & ~c.stats, FUSED], \
            [(c.mode == BOX) & c.stats, TRACE_SHADE]
    covered = np.zeros(c.n, bool)
    for rows, kernel in table:
        check(c, ~(v0 & rows) | (c.kernel == kernel), f"default build, kernel {kernel}")
        covered |= rows
    assert covered.all()
    check(c, ~((c.bits == 32768) & c.prim & ~c.generic) | (c.kernel == TRACE_SHADE), "32768: trace + shade")
    check(c, ~(c.bits == 65536) | ((c.kernel == GENERIC) == (c.mode != BOX)), "65536: generic except box colours")
    # every variant, by the kernel list of rt_dispatch.h; with stats always the counting trace kernel, even under
    # 256 / 2048
    unfused = (c.bits & (32768 | 256 | 2048)) != 0
    want = np.select(
        [c.generic, c.dual, (c.mode == FULL) & ((c.bits & 16) != 0), c.mode == FULL, ~c.stats & ~unfused & c.lds,
         c.stats | ~c.lds, (c.bits & 256) != 0, (c.bits & 2048) != 0],
        [GENERIC, DUAL, PIPELINE, MEGAKERNEL, FUSED, TRACE_SHADE, TWO_RAYS, PERSISTENT], TRACE_SHADE)
    check(c, c.kernel == want, "kernel")
    check(c, c.units == np.where(want == DUAL, 2, 4) * c.slots, "units")
    # the refusal test_wave_stats_sum_to_frame_counters sees on the GPU
    check(c, c.writes_wave_stats == (want != GENERIC), "writes_wave_stats")
    check(c, c.pipeline_buffers == ((c.mode == FULL) & ((c.bits & 16) != 0)), "pipeline_buffers")


def test_empty_shard_launches_nothing(rt):
    p = rt.frame_plan(FULL, 3, 0, 1, 1, 7, 8, 0, SMALL, False, True)  # one super-tile: shard 7 of 8 has no tiles
    assert p["kernel"] == NONE and p["grid"] == 0 and p["units"] == 0 and p["lpt"] == 0 and p["split_ceiling"] == 0
    assert p["writes_wave_stats"] == 0  # still the generic-depth frame it would be


def test_block_order_and_longest_first(c):
    check(c, c.l2_resident == c.small, "l2_resident")
    runs = c.bits & 1536
    want = np.select([(c.bits & 4) != 0, runs == 512, runs == 1024, runs == 1536, c.small], [1, 4, 16, 0, 64],
                     np.maximum(2, c.units // 8))
    check(c, c.xcd_remap == want, "xcd_remap")
    check(c, c.rotate_bands == ((c.alone == 0) & ~c.small & (want >= 2)), "rotate_bands")
    lpt = c.lpt != 0
    check(c, ~lpt | (np.isin(c.kernel, (GENERIC, FUSED, DUAL, MEGAKERNEL)) & ~c.stats & (c.xcd_remap >= 2) & (c.grid > 0) &
                     ((c.bits & NO_LPT) == 0) & ((c.alone != 0) | ((c.bits & LPT_IN_FLIGHT) != 0))), "lpt implies")
    # the default build dispatches exactly its lone frames longest-first
    check(c, ~((c.bits == 0) & ~c.stats) | (lpt == (c.alone != 0)), "lpt, default build")
    check(c, ~((c.bits == LPT_IN_FLIGHT) & ~c.stats) | lpt, "lpt, 524288")
    check(c, ~(c.bits == NO_LPT) | ~lpt, "lpt, 131072")


def test_wave_split_ceiling(c):
    k = c.split_ceiling
    # the FULL megakernel splits by the build it runs: its small-scene build, which 16384 / 8192 force on / off
    check(c, c.full_small_build == (((c.bits & 16384) != 0) | (((c.bits & 8192) == 0) & c.small)), "full_small_build")
    splits_large = (c.kernel == MEGAKERNEL) & ((c.bits & 16384) != 0)
    check(c, c.small | splits_large | (k == 0), "a large scene splits")
    check(c, (k % 8 == 0) & (k >= 0) & (k <= c.units // 4), "ceiling: a multiple of 8, at most a quarter of the waves")
    check(c, (k == 0) | (np.isin(c.kernel, (FUSED, MEGAKERNEL)) & ~c.stats), "only the fused kernel and the megakernel split")
    # 24x16, 8 waves: test_split_costliest_waves relies on no split here
    tiny = (c.tiles_x == 2) & (c.tiles_y == 1) & (c.shards == 1)
    check(c, ~tiny | ((c.units <= 8) & (k == 0)), "24x16 splits")
    hd = (c.bits == 0) & c.small & ~c.stats & (c.tiles_x == 120) & (c.tiles_y == 68) & (c.shards == 1)
    check(c, ~(hd & (c.kernel == FUSED)) | (k == 256), "kSplitKPrimary")
    check(c, ~(hd & (c.kernel == MEGAKERNEL)) | (k == 1536), "kSplitK")
