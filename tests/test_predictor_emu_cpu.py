"""CPU self-test of the predictor's bf16 emulation (oracle.predictor_forward_emu) and of the layer bounds tests/test_predictor_gpu.py
asserts with it.

The emulation is pinned to the fp32 oracle with rounding off, and teacher forcing with its own taps must change nothing.  Then a
"correct kernel" stand-in (the emulation's own activations, bf16-rounded like the stored ones) gets one modelled fault in one
activation, and the teacher-forced emulation is compared with it layer by layer exactly as the GPU test compares the HIP path: the
faulty layer must fail the layer bounds, and the correct layers before it must pass them.  The same fault carried through the rest of the
network is also compared with the fp32 oracle under test_predictor's end-to-end bound (1.5e-2), to record which faults only the
layer-wise check sees.
"""
import pytest
import torch
import torch.nn.functional as F

import hip_checks as C
from oracle import ucdir_oracle as O
from ucdir_amd.spec import UNetConfig
from ucdir_amd.weights import synth_inputs, synth_state_dict

E2E_TOL = 1.5e-2       # test_predictor's end-to-end bound against the fp32 oracle (tests/test_hip_gpu.py)
SHAPE = (1, 64, 96)    # padded to 96 x 128: 6 x 8 at the deepest level


@pytest.fixture(scope="module")
def sd():
    cfg = UNetConfig(inner_channel=64, channel_mults=(1, 2), res_blocks=1, attn_res=(64,), image_size=128)
    full = O.to_torch_sd(synth_state_dict(cfg, 0))
    return {k: v for k, v in full.items() if k.startswith("predictor.")}


@pytest.fixture(scope="module")
def x():
    return torch.from_numpy(synth_inputs(*SHAPE, seed=3)[0])


def test_emulation_without_rounding_is_the_oracle(sd, x):
    ref = O.predictor_forward(sd, x)
    taps = {}
    e = O.predictor_forward_emu(sd, x, taps=taps, rnd=False)
    assert C.metrics(e, ref)["rel_rms"] <= 1e-6
    names = C.PREDICTOR_LAYERS
    assert set(taps) == set(names), set(taps) ^ set(names)
    # teacher forcing with its own values is the identity
    again = O.predictor_forward_emu(sd, x, force=dict(taps), rnd=False)
    assert torch.equal(again, e)
    taps_r = {}
    er = O.predictor_forward_emu(sd, x, taps=taps_r)
    assert torch.equal(O.predictor_forward_emu(sd, x, force=dict(taps_r)), er)
    # the rounding plan itself stays within test_predictor's bound of the fp32 oracle
    assert C.metrics(er, ref)["rel_rms"] < E2E_TOL


def _slope(sd, stand, name, slope):
    """``name`` recomputed from the stand-in's own input with LeakyReLU slope ``slope`` instead of 0.2."""
    lvl = int(name[4])
    src = {1: None, 2: "pool1", 3: "pool2", 4: "pool3", 5: "pool4"}.get(lvl) if name.endswith("_1") else f"conv{lvl}_1"
    assert src is not None and lvl <= 5
    pre = F.conv2d(C.bfr(stand[src]), C.bfr(sd[f"predictor.{name}.weight"]), sd[f"predictor.{name}.bias"], padding=1)
    return C.bfr(torch.max(slope * pre, pre))


def _faults(sd, x, stand):
    """{fault: (layer, faulty bf16 activation)}."""
    out = {}
    y = stand["upv7"].clone()                          # pixel shuffle: sub-pixel phases (0, 1) and (1, 0) of every pixel swapped
    y[..., 0::2, 1::2], y[..., 1::2, 0::2] = stand["upv7"][..., 1::2, 0::2], stand["upv7"][..., 0::2, 1::2]
    out["upv_phase_swap"] = ("upv7", y)
    B, _, H, W = x.shape                               # stem: the last padded row reflected about row H instead of H - 1
    ph, pw = O.pad32(H), O.pad32(W)
    xp = F.pad(x, (0, pw, 0, ph), mode="reflect")
    Hc = H + ph
    xp[..., Hc - 1, :] = F.pad(x, (0, pw, 0, 0), mode="reflect")[..., 2 * H - (Hc - 1), :]
    b1 = sd["predictor.conv1_1.bias"]
    b1 = C.bfr(b1) + C.bfr(b1 - C.bfr(b1))
    pre = F.conv2d(C.bfr(xp), C.bfr(sd["predictor.conv1_1.weight"]), b1, padding=1)
    out["reflect_last_row"] = ("conv1_1", C.bfr(torch.max(0.2 * pre, pre)))
    out["slope_0.25"] = ("conv3_2", _slope(sd, stand, "conv3_2", 0.25))
    return out


def test_modelled_faults_fail_the_layer_bounds(sd, x):
    taps = {}
    O.predictor_forward_emu(sd, x, taps=taps)
    stand = {k: C.bfr(v) for k, v in taps.items()}     # a correct kernel: the emulation's own values, stored as bf16
    ref = O.predictor_forward(sd, x)
    passes_e2e = {}
    for fault, (layer, bad) in _faults(sd, x, stand).items():
        assert not torch.equal(bad, stand[layer]), fault
        force = dict(stand)
        force[layer] = bad
        etaps = {}
        O.predictor_forward_emu(sd, x, taps=etaps, force=force)
        for k in C.PREDICTOR_LAYERS[:C.PREDICTOR_LAYERS.index(layer) + 1]:
            m = C.metrics(force[k], C.bfr(etaps[k]))
            if k == layer:                             # the faulty layer fails the bounds the GPU test asserts
                assert not C.emu_layer_ok(m), (fault, k, m)
                assert m["tile_max"] > 2 * C.EMU_TILE_TOL, (fault, k, m)
            else:                                      # the correct layers before it pass them
                assert C.emu_layer_ok(m), (fault, k, m)
        # the fault carried through the rest of the network, against the fp32 oracle under test_predictor's old bound
        e2e = O.predictor_forward_emu(sd, x, force={layer: bad})
        r = C.metrics(e2e, ref)["rel_rms"]
        print(fault, "end to end", r)
        passes_e2e[fault] = r < E2E_TOL
    print("faults that still pass the end-to-end bound:", passes_e2e)
    assert passes_e2e == EXPECT_E2E, passes_e2e


# Which modelled faults the old end-to-end bound alone lets through at SHAPE (deterministic on CPU; measured end-to-end rel-RMS:
# phase swap 0.255, last reflect row 7.0e-3, slope 0.25 in conv3_2 2.2e-2).  The reflect fault touches two of 96 padded rows and is
# cropped away with the pad; at a larger image its share, and so its end-to-end error, only shrinks.
EXPECT_E2E = {"upv_phase_swap": False, "reflect_last_row": True, "slope_0.25": False}
