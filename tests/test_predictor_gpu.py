"""The UNetSeeInDark predictor on the HIP engine layer by layer (``pytest -m gpu``).

Its output is the guide of every denoiser call and the residual base of the restored image, so an error in it reaches every
pixel.  Every named activation (conv{l}_1 / conv{l}_2 after LeakyReLU, pool{l}, upv{l}) is compared with
oracle.predictor_forward_emu fed with the HIP path's own activations (teacher forcing), under the denoiser's layer bounds, at the
sizes the product runs it: the minimum size, odd sizes, a 256^2 val image after DDPM.test's pad of 64 (B = 1 and sr.py's batch of
16) and configs[2]'s full image (1552 x 2256, padded to 1568 x 2272).  tests/test_predictor_emu_cpu.py shows that a swapped
pixel-shuffle phase, a wrong reflect row and a LeakyReLU slope error in one layer fail these bounds.

Kernels reached (profiler keys, hip_checks.profile_keys; the stem and maxpool are launched directly and not profiled): the
LeakyReLU epilogue of conv3x3_halo (20 / 120; its split-K finish kernel runs inside key 20 / 120 where the grid is small), conv_ws
(23), conv_sk (127, 129) and the cgemm launches (0 / 100: upv and conv10_1, which carry NO activation).  conv_sk's persistent 8-wave
kind (125) and conv_ws128 (24) never run in the predictor: the engine picks kind 125 only when forced, and conv_ws128 only for a
fused res_conv.  The operator tests (test_hip_gpu.py::test_conv_leaky_relu_epilogue) cover act 2 on every family, those included.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402
from oracle import ucdir_oracle as O  # noqa: E402
from ucdir_amd import lib as ulib  # noqa: E402
from ucdir_amd.spec import UNetConfig  # noqa: E402
from ucdir_amd.weights import synth_inputs  # noqa: E402

NET_CFG = UNetConfig(inner_channel=64, channel_mults=(1, 2), res_blocks=1, attn_res=(64,), image_size=128)

SHAPES = [(1, 33, 33), (2, 64, 96), (3, 45, 77), (1, 384, 384), (16, 384, 384), (1, 1552, 2256)]
IDS = ["min33", "b2_64x96", "odd_b3", "val256", "val256_b16", "configs2_full"]
# profiler keys each shape produced on the MI355X (256 CUs): up to 384^2 at B = 1 every 3x3 conv is conv3x3_halo at TM = 64 (the
# deep levels split-K); sr.py's batch of 16 and the full image reach conv_ws (64 -> 64 at level 1), conv3x3_halo at TM = 128 and
# conv_sk; the mixed schedule only at B = 16
SMALL_KEYS = {20, 100, 0}
EXPECT_KEYS = {(1, 33, 33): SMALL_KEYS, (2, 64, 96): SMALL_KEYS, (3, 45, 77): SMALL_KEYS, (1, 384, 384): SMALL_KEYS,
               (16, 384, 384): {23, 120, 127, 129, 20, 100, 0}, (1, 1552, 2256): {23, 120, 127, 20, 100, 0}}
# across the shapes, every conv family that carries the predictor's LeakyReLU runs: conv3x3_halo (20 / 120, split-K inside the same
# key), conv_ws (23), conv_sk (127 / 129), and the cgemm launches of upv / conv10_1 (0 / 100)
assert set(EXPECT_KEYS) == set(SHAPES)
assert all(k in set().union(*EXPECT_KEYS.values()) for k in (20, 120, 23, 127, 129, 0, 100))


@pytest.fixture(scope="module")
def net_sd():
    return C.build_net(NET_CFG)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_predictor_layer_by_layer_vs_emulation(net_sd, shape):
    net, sd = net_sd
    L = ulib.load()
    (res, got, x), keys = C.profile_keys(L, lambda: C.predictor_emu_case(net, sd, *shape))
    worst = {b: max(v.items(), key=lambda kv: kv[1]["rel_rms"]) for b, v in res["samples"].items()}
    worst_tile = {b: max(v.items(), key=lambda kv: kv[1]["tile_max"]) for b, v in res["samples"].items()}
    print(shape, "keys", keys)
    print(shape, "worst rel_rms", {b: (k, m["rel_rms"]) for b, (k, m) in worst.items()})
    print(shape, "worst tile_max", {b: (k, m["tile_max"], m["elem_max"]) for b, (k, m) in worst_tile.items()})
    print(shape, "worst elem_max", max((m["elem_max"], b, k) for b, v in res["samples"].items() for k, m in v.items()))
    assert res["out_finite"]
    assert all(res["finite"].values()), res["finite"]
    assert set(res["finite"]) == set(C.PREDICTOR_LAYERS)
    # the 32-channel layers carried as 64: upper half exactly zero
    assert set(res["upper"]) == {"conv1_1", "conv1_2", "pool1", "upv9", "conv9_1", "conv9_2"}, res["upper"]
    assert all(v == 0.0 for v in res["upper"].values()), res["upper"]
    for b, layers in res["samples"].items():
        assert set(layers) == set(C.PREDICTOR_LAYERS) | {"out"}
        for k, m in layers.items():
            assert C.emu_layer_ok(m), (shape, b, k, m)
    assert keys.keys() == EXPECT_KEYS[tuple(shape)], keys


def test_predictor_replans_bit_identically_and_rejects_small_images(net_sd):
    net, _ = net_sd
    pred = net.predictor

    def run(B, H, W, seed=5):
        x = torch.from_numpy(synth_inputs(B, H, W, seed=seed)[0]).cuda()
        with torch.no_grad():
            y = pred(x)
        torch.cuda.synchronize()
        return y.cpu()

    a = run(2, 64, 96)
    assert torch.equal(run(2, 64, 96), a)                  # the same input twice
    b = run(3, 45, 77)
    assert torch.equal(run(2, 64, 96), a)                  # back after a re-plan
    c = run(1, 64, 96)
    assert torch.equal(run(2, 64, 96), a)
    assert torch.equal(run(3, 45, 77), b)
    assert torch.equal(run(1, 64, 96), c)
    # each bad shape twice in a row: a rejection that half-applied its plan (shape recorded, activations released) made the
    # second call skip planning and fail on the missing activations with another message
    for bad in [(2, 32, 96), (2, 32, 96), (2, 64, 32), (2, 64, 32)]:
        with pytest.raises(ulib.UcdirError, match=r"predictor: H, W must be >= 33 \(reflect pad\)"):
            run(*bad)
    assert torch.equal(run(1, 64, 96), c)                  # straight after: the last good plan (1, 64, 96) is intact
    assert torch.equal(run(2, 64, 96), a)
    with pytest.raises(KeyError):
        pred.debug_read("conv10_1")
    L = ulib.load()
    out = torch.empty(4, device="cuda")
    with pytest.raises(ulib.UcdirError, match="unknown predictor activation"):
        ulib.check(L.ucdir_predictor_debug_read(pred._handle(), b"conv0_1", C._p(out), 4, C._st()))
    with pytest.raises(ulib.UcdirError, match="predictor_debug_read: dst has"):
        ulib.check(L.ucdir_predictor_debug_read(pred._handle(), b"conv1_1", C._p(out), 4, C._st()))
    # the end-to-end result of the odd shape against the fp32 oracle
    _, sd = net_sd
    m = C.metrics(b, O.predictor_forward(sd, torch.from_numpy(synth_inputs(3, 45, 77, seed=5)[0])))
    assert m["rel_rms"] < 1.5e-2, m
