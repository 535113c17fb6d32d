"""CPU tests of the sampler's noise contract: the float64 host reference of the in-kernel Philox stream (oracle.philox_normal)
against the Random123 known answers, the properties include/ucdir_hip.h states, a table of modelled kernel faults that the GPU bound
of tests/test_noise_stream_gpu.py must catch, and the two host pieces every rank's stream depends on (the per-sample key tensor of
GaussianDiffusion and sr.py's seed base)."""
import math
import os

import numpy as np
import pytest
import torch

import hip_checks as C
from oracle import ucdir_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1
Z_MAX = math.sqrt(-2.0 * math.log(2.0 ** -24))          # the smallest uniform is 0.5 * 2^-23: |z| <= 5.768


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds, one at a time and as one row of a vectorised call."""
    assert tuple(int(v) for v in O.philox4x32_10(ctr, key)) == want
    rows = O.philox4x32_10(np.array([ctr, (1, 2, 3, 4), ctr], dtype=np.uint64), np.array([key, key, key], dtype=np.uint64))
    assert tuple(int(v) for v in rows[2]) == want and tuple(int(v) for v in rows[0]) == want


# ---- the stream --------------------------------------------------------------------------------------------------------------------
def test_uniforms_lie_strictly_inside_the_unit_interval_and_bound_z():
    ends = O.philox_u23([0, 0xFFFFFFFF])
    assert ends[0] == 2.0 ** -24 and ends[1] == 1.0 - 2.0 ** -24
    assert np.array_equal(ends.astype(np.float32).astype(np.float64), ends)         # exact in the kernel's fp32 too
    words = O.philox4x32_10(np.stack([np.arange(1 << 16), np.zeros(1 << 16), np.full(1 << 16, 5), np.full(1 << 16, O.PHILOX_TAG)], -1),
                            [1234, 0])
    u = O.philox_u23(words)
    assert 0.0 < u.min() and u.max() < 1.0
    z = O.philox_normal(1 << 18, 1234, 5)
    assert np.abs(z).max() <= Z_MAX
    assert abs(z.mean()) < 1e-2 and abs(z.var() - 1.0) < 1e-2
    assert math.sqrt(-2.0 * math.log(ends[0])) == pytest.approx(Z_MAX, abs=1e-12)


def test_element_depends_on_seed_step_and_index_only():
    a = O.philox_normal(4096, 2 ** 32 + 7, 49)
    for n in (1, 3, 5, 1027):
        assert np.array_equal(O.philox_normal(n, 2 ** 32 + 7, 49), a[:n])
    assert np.array_equal(O.philox_normal(1024, 2 ** 32 + 7, 49, first=2048), a[2048:3072])
    for other in (O.philox_normal(4096, 2 ** 32 + 8, 49), O.philox_normal(4096, 7, 49), O.philox_normal(4096, 2 ** 32 + 7, 50)):
        assert np.abs(other - a).max() > 1.0
    # the seed is its uint64 bit pattern; the step one 32-bit word
    assert np.array_equal(O.philox_normal(64, -3, 2), O.philox_normal(64, 2 ** 64 - 3, 2))
    assert np.array_equal(O.philox_normal(64, 9, 2 ** 32 + 1), O.philox_normal(64, 9, 1))
    # the counter's high word (group >= 2^32; the GPU tests cannot reach it: buffers above 2^34 elements)
    hi = O.philox_normal(8, 11, 3, first=4 << 32)
    r = O.philox4x32_10([0, 1, 3, O.PHILOX_TAG], [11, 0])
    u = O.philox_u23(r)
    rad = math.sqrt(-2.0 * math.log(u[0]))
    assert hi[0] == pytest.approx(rad * math.cos(2 * math.pi * u[1]), abs=1e-15)
    assert hi[1] == pytest.approx(rad * math.sin(2 * math.pi * u[1]), abs=1e-15)
    assert np.abs(hi - O.philox_normal(8, 11, 3)).max() > 0.1


def test_batched_sample_equals_the_single_stream_of_its_seed():
    seeds = [0, 2 ** 63 + 5, M64, -3, 1234]
    per = 3 * 40 * 56
    z = O.philox_normal(per * len(seeds), 0, 7, per=per, seeds=seeds)
    for b, s in enumerate(seeds):
        assert np.array_equal(z[b * per:(b + 1) * per], O.philox_normal(per, s, 7))
    with pytest.raises(ValueError):
        O.philox_normal(30, 0, 7, per=6, seeds=[1, 2, 3, 4, 5])


# ---- modelled kernel faults ----------------------------------------------------------------------------------------------------------
def _stream(n, seed, step, words=None, key=None, pairs=((0, 1), (2, 3)), revolutions=True, sin_cos=False, group0=0):
    """philox_normal with one piece of its statement changed: counter ``words`` / ``key`` as functions of (g, step, seed), the
    Box-Muller word ``pairs``, the angle in radians, sin and cos exchanged, or the group index offset by ``group0``."""
    seed &= M64
    g = np.arange(group0, group0 + (n + 3) // 4, dtype=np.uint64)
    lo, hi = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    step_w, tag = np.full_like(g, step & 0xFFFFFFFF), np.full_like(g, O.PHILOX_TAG)
    ctr = np.stack((words or (lambda lo, hi, s, t: (lo, hi, s, t)))(lo, hi, step_w, tag), -1)
    u = O.philox_u23(O.philox4x32_10(ctr, (key or (lambda s: (s & 0xFFFFFFFF, s >> 32)))(seed)))
    z = np.empty(u.shape)
    for j, (a, b) in enumerate(pairs):
        rad, ang = np.sqrt(-2.0 * np.log(u[:, a])), u[:, b] * (2 * np.pi if revolutions else 1.0)
        c, s = np.cos(ang), np.sin(ang)
        z[:, 2 * j], z[:, 2 * j + 1] = (s, c) if sin_cos else (c, s)
        z[:, 2 * j:2 * j + 2] *= rad[:, None]
    return z.reshape(-1)[:n]


SEED, STEP, N = 2 ** 32 + 7, 49, 4096
FAULTS = {
    "key_words_swapped": lambda: _stream(N, SEED, STEP, key=lambda s: (s >> 32, s & 0xFFFFFFFF)),
    "counter_words_swapped": lambda: _stream(N, SEED, STEP, words=lambda lo, hi, s, t: (hi, lo, s, t)),
    "step_in_the_tag_word": lambda: _stream(N, SEED, STEP, words=lambda lo, hi, s, t: (lo, hi, t, s)),
    "step_in_the_high_group_word": lambda: _stream(N, SEED, STEP, words=lambda lo, hi, s, t: (lo, s, hi, t)),
    "tag_word_dropped": lambda: _stream(N, SEED, STEP, words=lambda lo, hi, s, t: (lo, hi, s, 0 * t)),
    "angle_in_radians": lambda: _stream(N, SEED, STEP, revolutions=False),
    "sin_and_cos_swapped": lambda: _stream(N, SEED, STEP, sin_cos=True),
    "word_pairs_r0r2_r1r3": lambda: _stream(N, SEED, STEP, pairs=((0, 2), (1, 3))),
    "step_off_by_one": lambda: _stream(N, SEED, STEP + 1),
    "seed_reduced_mod_2_63": lambda: _stream(N, (2 ** 63 + 5) % 2 ** 63, STEP),   # the old per-sample key of GaussianDiffusion._seeds_tensor
}


def test_reference_restatement_is_the_unfaulted_variant():
    assert np.array_equal(_stream(N, SEED, STEP), O.philox_normal(N, SEED, STEP))


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_every_modelled_fault_exceeds_the_gpu_bound(fault):
    """Each fault changes the stream by orders of magnitude more than the |dz| the GPU tests allow (hip_checks.NOISE_Z_TOL)."""
    ref = O.philox_normal(N, 2 ** 63 + 5 if fault == "seed_reduced_mod_2_63" else SEED, STEP)
    d = np.abs(FAULTS[fault]() - ref)
    print(fault, "max |dz| %.3g, rms %.3g, share of elements above the bound %.3f" % (d.max(), np.sqrt((d ** 2).mean()),
                                                                                      (d > C.NOISE_Z_TOL).mean()))
    assert d.max() > 1e5 * C.NOISE_Z_TOL and np.sqrt((d ** 2).mean()) > 1e5 * C.NOISE_Z_TOL
    assert (d > C.NOISE_Z_TOL).mean() > 0.9                   # nearly every element is off, not a few


def test_per_sample_counters_that_do_not_restart_exceed_the_gpu_bound():
    seeds, per = [11, 2 ** 40 + 5, 2 ** 63 + 5], 1024
    ref = O.philox_normal(per * 3, 0, STEP, per=per, seeds=seeds)
    bad = np.concatenate([_stream(per, s, STEP, group0=b * per // 4) for b, s in enumerate(seeds)])
    assert np.array_equal(bad[:per], ref[:per])                     # sample 0 is unaffected ...
    d = np.abs(bad[per:] - ref[per:])
    assert np.sqrt((d ** 2).mean()) > 1e5 * C.NOISE_Z_TOL and (d > C.NOISE_Z_TOL).mean() > 0.9   # ... every later one is off


# ---- host pieces ---------------------------------------------------------------------------------------------------------------------
def test_seeds_tensor_holds_each_seeds_uint64_bit_pattern():
    """GaussianDiffusion._seeds_tensor: the per-sample key of seed v is int(v) & (2^64 - 1) - what the single-stream wrappers
    (fill_normal_, sampler_step_rng_, fewstep_update_) pass - stored as the int64 of the same bits."""
    from ucdir_amd.diffusion import GaussianDiffusion
    gd = GaussianDiffusion.__new__(GaussianDiffusion)
    gd.noise_source = None
    seeds = [2 ** 63 + 5, M64, -3, 1234, 0, 2 ** 63 - 1, 2 ** 64 + 9]
    gd.sample_seeds = seeds
    t = gd._seeds_tensor(torch.zeros(len(seeds), 3, 4, 4))
    assert t.dtype == torch.int64 and t.device.type == "cpu"
    want = np.array([s & M64 for s in seeds], dtype=np.uint64).view(np.int64)
    assert t.tolist() == want.tolist()
    assert [v & M64 for v in t.tolist()] == [s & M64 for s in seeds]
    gd.sample_seeds = [1, 2]
    with pytest.raises(ValueError):
        gd._seeds_tensor(torch.zeros(3, 3, 4, 4))


def _seed_base_worker(rank, world, port, q):
    import importlib.util
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if rank == 1:
        torch.rand(1)                                    # this rank's CPU generator is one draw ahead
    spec = importlib.util.spec_from_file_location("sr_seed_base", os.path.join(ROOT, "sr.py"))
    sr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sr)
    state = torch.get_rng_state()
    own = int(torch.randint(0, 2 ** 31, (1,)).item())   # what this rank would draw on its own
    torch.set_rng_state(state)
    q.put((rank, (sr.image_seed_base(None), sr.image_seed_base(-5)), own))
    dist.barrier()
    dist.destroy_process_group()


def test_image_seed_base_is_rank_zeros_on_every_rank_gloo():
    """sr.py's per-image seed base: one value on every rank even when one rank's CPU generator has been consumed before."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    from conftest import free_port
    port = free_port()
    procs = [ctx.Process(target=_seed_base_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (bases, own) for r, bases, own in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(60)
    (b0, own0), (b1, own1) = got[0], got[1]
    assert own0 != own1, got                             # the ranks' own draws differ ...
    assert b0 == b1 == (own0, -5), got                   # ... and both take rank 0's; an explicit --seed is taken as given
