"""GPU sweep over the pixel tiles the engine's choose_tile can pick (``pytest -m gpu``): conv3x3_halo, its Upsample parity
launches and the one-shot AKGM kernels decode slot -> (row, column) with the tile's width, clamp its halo at the plane's edge
and mask its ragged stores, so every one of them depends on (th, tw).  hip_checks.tile_cover gives 207 of the 614 distinct
tiles of the planes up to 112 x 112 - both extremes of tw for every th and of th for every tw, every tile near the
324-position halo limit, every 256-position tile - each with the smallest plane that yields it with two tiles along both axes
where such a plane exists (tests/test_small_shapes_cpu.py checks the cover and the copy of choose_tile against the library).
Every plane runs at B = 2 through each kernel family against torch, with the single-operator bounds and the profiler key of
the kernel meant.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402

OP_TOL = 4e-3          # single operator, bf16-representable inputs (tests/test_hip_gpu.py)
COVER = C.tile_cover(2, 112)
_ids = [f"t{th}x{tw}_p{H}x{W}" for (th, tw), (H, W) in COVER]
cover = pytest.mark.parametrize("case", COVER, ids=_ids)


def _tile_is(th, tw, H, W):
    assert C.ulib.load().ucdir_debug_launch_plan(b"tile", H, W, 0, 0.0) == th * 1000 + tw, (th, tw, H, W)


def _conv_ok(m):
    assert C.op_ok(m, OP_TOL), m
    assert m["max_abs_border"] < 0.05 * max(m["ref_rms"], 1.0), m
    assert m["stats_rel"] < 1e-3, m


def _akgm(B, Cc, H, W, key):
    m, keys = C.profile_keys(C.ulib.load(), lambda: C.akgm_case(B, Cc, H, W, seed=43))
    print((B, Cc, H, W), keys, m)
    assert keys.keys() == {key}, keys
    assert C.op_ok(m, OP_TOL), m
    assert m["max_abs_border"] < 0.06, m
    assert m["stats_rel"] < 1e-3, m


@cover
def test_conv_halo_on_every_tile_shape(case):
    """conv3x3_halo_kernel<64> (64 -> 64, GroupNorm fold + swish, key 20)."""
    (th, tw), (H, W) = case
    _tile_is(th, tw, H, W)
    m, keys = C.profile_keys(C.ulib.load(), lambda: C.conv_case(2, H, W, 64, 0, 64, 3, 0, True, True, False, seed=41))
    print(case, keys, m)
    assert keys.keys() == {20}, keys
    _conv_ok(m)


@cover
def test_upsample_parity_launches_on_every_tile_shape(case):
    """The Upsample parity launches of conv3x3_halo_kernel<64> (64 -> 64, key 21): tiles on the low-resolution grid, stores
    on the 2 H x 2 W one."""
    (th, tw), (H, W) = case
    _tile_is(th, tw, H, W)
    m, keys = C.profile_keys(C.ulib.load(), lambda: C.conv_case(2, H, W, 64, 0, 64, 3, 2, False, False, False, seed=42))
    print(case, keys, m)
    assert keys.keys() == {21}, keys
    _conv_ok(m)


@cover
def test_akgm_pre_on_every_tile_shape(case):
    """akgm_pre_kernel<8> (C = 64, key 112)."""
    (th, tw), (H, W) = case
    _tile_is(th, tw, H, W)
    _akgm(2, 64, H, W, 112)


@cover
def test_akgm_halo_on_every_tile_shape(case):
    """akgm_halo_kernel (C = 128, 16 channels per group, key 111)."""
    (th, tw), (H, W) = case
    _tile_is(th, tw, H, W)
    _akgm(2, 128, H, W, 111)


@cover
def test_akgm_halo_stage_on_every_tile_shape(case):
    """akgm_halo_stage_kernel (C = 512, key 111) with the engine's own dispatch (no forced grid).  On this device's CU count
    akgm_ws64 takes some of the larger planes at B = 2 by its own rule (hip_checks.ws64_tile: 13 of the cover's planes on 256
    CUs); the tile then runs on the smallest plane that yields it and stays with the one-shot kernel, so that every tile of
    the cover meets akgm_halo_stage."""
    (th, tw), (H, W) = case
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if C.ws64_tile(2, H, W, ncu):
        hw = C.tile_plane((th, tw), admit=lambda p: not C.ws64_tile(2, p[0], p[1], ncu))
        assert hw is not None, (case, ncu)
        print(f"tile {th} x {tw}: akgm_ws64 takes {H} x {W} at B = 2 on {ncu} CUs; plane {hw[0]} x {hw[1]} instead")
        H, W = hw
    _tile_is(th, tw, H, W)
    _akgm(2, 512, H, W, 111)
