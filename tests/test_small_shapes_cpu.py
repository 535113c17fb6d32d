"""Host-side checks behind the smallest-shape GPU tests (tests/test_small_planes_gpu.py, test_tile_cover_gpu.py,
test_small_denoiser_gpu.py): the Python copies of the engine's pixel-tile choice and of conv_sk's strip rule against the
library itself (ucdir_debug_launch_plan needs no device), the tile cover built from them, and the emulation against itself
with a second summation order at the smallest denoiser shapes - the measurement the block-size condition of EMU_TILE_TOL
(hip_checks.EMU_TILE_MIN_BLOCK) rests on.
"""
import pytest
import torch

import hip_checks as C
from ucdir_amd import lib as ulib
from ucdir_amd.spec import UNetConfig
from ucdir_amd.weights import synth_state_dict

SID = UNetConfig(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=2, attn_res=(16,), image_size=128)
HALO_LIMIT_TILES = {(16, 16), (10, 25), (25, 10), (7, 34), (34, 7), (52, 4), (4, 52), (2, 79)}


def test_choose_tile_copy_is_the_librarys():
    """hip_checks.choose_tile against the engine's choose_tile for every plane with H, W in 2..160, and the tile's own limits."""
    plan = ulib.load().ucdir_debug_launch_plan
    bad = []
    for H in range(2, 161):
        for W in range(2, 161):
            th, tw = C.choose_tile(H, W)
            if plan(b"tile", H, W, 0, 0.0) != th * 1000 + tw:
                bad.append((H, W, (th, tw), plan(b"tile", H, W, 0, 0.0)))
            assert 1 <= th <= 64 and 4 <= tw <= 256 and th * tw <= 256 and (th + 2) * (tw + 2) <= C.HALO_PX, (H, W, th, tw)
    assert not bad, bad[:10]
    assert plan(b"tile", 0, 5, 0, 0.0) == -1 and plan(b"tile", 5, 0, 0, 0.0) == -1


def test_tile_cover():
    """The distinct tiles of the planes with H, W in 2..112 and the cover the GPU sweep runs: both extremes of tw for every
    th and of th for every tw, every tile near the 324-position halo limit, every 256-position tile; each with a plane that
    yields it (two tiles along both axes where such a plane exists)."""
    tm = C.tile_map(2, 112)
    tiles = set(tm.values())
    cover = C.tile_cover(2, 112)
    ct = {t for t, _ in cover}
    print(f"{len(tiles)} distinct tiles, {len({t[0] for t in tiles})} values of th, tw {min(t[1] for t in tiles)}.."
          f"{max(t[1] for t in tiles)}; cover: {len(cover)} tiles")
    assert len(tiles) == 614 and len({t[0] for t in tiles}) == 51
    assert (min(t[1] for t in tiles), max(t[1] for t in tiles)) == (4, 79)
    assert {t for t in tiles if (t[0] + 2) * (t[1] + 2) == C.HALO_PX} == HALO_LIMIT_TILES
    assert len(cover) == 207 and len(ct) == 207 and ct <= tiles and HALO_LIMIT_TILES <= ct
    assert {t[0] for t in ct} == {t[0] for t in tiles} and {t[1] for t in ct} == {t[1] for t in tiles}
    assert {t for t in tiles if t[0] * t[1] == 256 or (t[0] + 2) * (t[1] + 2) >= 300} <= ct
    two = {2: 0, 1: 0, 0: 0}
    for (th, tw), (H, W) in cover:
        assert tm[H, W] == (th, tw)
        n = (-(-H // th) >= 2) + (-(-W // tw) >= 2)
        two[n] += 1
        assert n == max((-(-h // th) >= 2) + (-(-w // tw) >= 2) for (h, w), t in tm.items() if t == (th, tw))
    print("planes with two tiles along both axes / one axis / a single tile:", two[2], two[1], two[0],
          " largest plane:", max(h * w for _, (h, w) in cover), "positions")
    assert two[2] > 0


@pytest.mark.parametrize("kind", [(1, 4), (2, 8), (1, 8)], ids=["sk_1_4", "sk_2_8", "sk_1_8"])
def test_conv_sk_strip_rule_copy_is_the_librarys(kind):
    """hip_checks.conv_sk_strips against the engine's conv_sk_strips<MW, NW> for every width up to 1024, and the widths at
    which the strip count changes (the GPU tests run both sides of each): CvSk<1, 4> holds one strip up to W = 54, two from 55
    and three from 107."""
    MW, NW = kind
    plan = ulib.load().ucdir_debug_launch_plan
    for W in range(1, 1025):
        r = C.conv_sk_strips(MW, NW, W)
        assert plan(b"sk_strips", W, 10 * MW + NW, 0, 0.0) == (r[0] * 1000 + r[1] if r else 0), (W, r)
    sw = C.conv_sk_strip_switches(MW, NW)
    print(f"CvSk<{MW}, {NW}>: strip count changes at", sw)
    assert len(sw) >= 2 and all(C.conv_sk_strips(MW, NW, a)[0] != C.conv_sk_strips(MW, NW, b)[0] for a, b in sw)
    assert [C.conv_sk_strips(MW, NW, b)[0] for _, b in sw[:2]] == [2, 3]
    if kind == (1, 4):
        assert sw[:2] == [(54, 55), (106, 107)], sw
    assert plan(b"sk_strips", 40, 15, 0, 0.0) == -1


@pytest.fixture(scope="module")
def sid_sd():
    from oracle import ucdir_oracle as O
    return O.to_torch_sd(synth_state_dict(SID, 0))


SELF_CASES = [((2, 32, 32), 31), ((3, 32, 64), 32), ((2, 64, 32), 33), ((2, 64, 64), 34)]
_self_cache = {}


def _self(sid_sd, shape, seed):
    if (shape, seed) not in _self_cache:
        torch.manual_seed(0)
        B, H, W = shape
        _self_cache[shape, seed] = C.emu_self_comparison(sid_sd, SID, B, H, W, [0.4, 0.003, 0.8][:B], seed)
    return _self_cache[shape, seed]


@pytest.mark.parametrize("shape,seed", SELF_CASES, ids=["2x32x32", "3x32x64", "2x64x32", "2x64x64"])
def test_emulation_against_itself_at_the_smallest_shapes(sid_sd, shape, seed):
    """Full SID configuration at the smallest compute sizes (level-4 planes of 2 x 2 ... 4 x 4): the emulation with fp32 sums
    against the emulation with float64 sums, every layer on the same stored activations.  What two correct implementations of
    the numerics plan differ by must fit the bounds the GPU tests assert at these shapes: EMU_LAYER_TOL and EMU_ELEM_TOL for
    every activation, EMU_TILE_TOL for those whose block holds >= EMU_TILE_MIN_BLOCK elements.  These four cases give rel_rms
    <= 3.7e-4, elem_max <= 2.3e-2, tile_max <= 4.5e-4 on blocks of >= 4096 elements and <= 6.9e-4 on smaller ones (the two
    orders differ by ~1e-7, so few outputs flip; test_one_flip_decides_the_tile_bound_on_a_small_block is about the size of
    a flip, not their number)."""
    out = _self(sid_sd, shape, seed)
    assert len(out) == 36 + 27 + 1, len(out)
    big = {k: m for k, m in out.items() if m.get("block", 0) >= C.EMU_TILE_MIN_BLOCK}
    small = {k: m for k, m in out.items() if 0 < m.get("block", 0) < C.EMU_TILE_MIN_BLOCK}
    wr = max(out, key=lambda k: out[k]["rel_rms"])
    we = max(out, key=lambda k: out[k]["elem_max"])
    wt = max(big, key=lambda k: big[k]["tile_max"])
    print(f"{shape}: worst rel_rms {out[wr]['rel_rms']:.3e} ({wr}), worst elem_max {out[we]['elem_max']:.3e} ({we}), worst tile_max on "
          f"blocks >= {C.EMU_TILE_MIN_BLOCK}: {big[wt]['tile_max']:.3e} ({wt})"
          + (f", on smaller blocks: {max(m['tile_max'] for m in small.values()):.3e}" if small else ""))
    assert big and small                                      # the shape has activations on both sides of the condition
    for k, m in out.items():
        assert C.emu_small_ok(m), (k, m)


def test_one_flip_decides_the_tile_bound_on_a_small_block(sid_sd):
    """Why EMU_TILE_TOL has a block-size condition.  Two correct summation orders differ in single outputs by one bf16 step
    (a "flip"): elem_max is the largest of them, relative to the activation's RMS, and a block of n elements that holds it has
    tile_max >= elem_max / sqrt(n) whatever else agrees.  Which output flips is chance - it depends on the last bits of an
    fp32 sum - so a bound for a block must leave room for the largest flip the numerics produce at these shapes.  The four
    self-comparisons give flips up to 2.2e-2 (an output of 3 - 6 RMS).  On the 256-element block of a 2 x 2 plane, which the
    GPU tests run, one such flip is 1.4e-3: above EMU_TILE_TOL, let alone two thirds of it.  On a block of EMU_TILE_MIN_BLOCK
    elements it is 3.5e-4, under half the bound, which is left to catch what it is for.  (On the MI355X, whose kernels sum
    in chunks and fold the GroupNorm into the conv, flips are more frequent and reach outputs of 7 - 14 RMS: 5.5e-2 on a
    512-element block of naiveforward 3 x 32 x 64 = 2.45e-3, with that activation's rel_rms and elem_max inside their bounds;
    hip_checks.EMU_TILE_MIN_BLOCK.)"""
    outs = [_self(sid_sd, shape, seed) for shape, seed in SELF_CASES]
    flip = max(m["elem_max"] for out in outs for m in out.values())
    blocks = {m["block"] for out in outs for m in out.values() if m.get("block", 0) > 0}
    print(f"largest flip {flip:.3e}; blocks {sorted(blocks)}; alone in the smallest block: {flip / min(blocks) ** 0.5:.3e}, in a block of "
          f"{C.EMU_TILE_MIN_BLOCK}: {flip / C.EMU_TILE_MIN_BLOCK ** 0.5:.3e}")
    assert min(blocks) == 256 and any(b >= C.EMU_TILE_MIN_BLOCK for b in blocks), blocks
    assert flip < C.EMU_ELEM_TOL
    assert flip / min(blocks) ** 0.5 > C.EMU_TILE_TOL                                  # unconditional, the bound would fail a correct layer
    assert all(flip / b ** 0.5 >= 2 / 3 * C.EMU_TILE_TOL for b in blocks if b <= 512)  # ... and is within a third of it at 512
    assert flip / C.EMU_TILE_MIN_BLOCK ** 0.5 < 0.5 * C.EMU_TILE_TOL                   # where it applies it has room
    # every measured tile_max is consistent with the relation the argument uses
    assert all(m["tile_max"] >= m["elem_max"] / m["block"] ** 0.5 * (1 - 1e-6) for out in outs for m in out.values() if m.get("block", 0) > 0)
