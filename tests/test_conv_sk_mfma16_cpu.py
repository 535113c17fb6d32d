"""Host-side check of conv_sk_kernel's halo swizzle for the 16 x 16 x 32 K loop (no device needed): a B fragment read takes 16
consecutive halo positions x the whole 64-byte pixel, and the library's brute-force bank check (ucdir_debug_launch_plan
"sk_halo_cycles": the ds_read_b128 lane groups over 64 banks, the kernel's own sk_halo_chunk) must give the conflict-free 4 LDS
cycles for every tap shift, every wave column and every row pitch of the position space a launch can have."""
from ucdir_amd import lib as ulib


def test_halo_fragment_reads_are_conflict_free():
    plan = ulib.load().ucdir_debug_launch_plan
    # row pitches: W + 1 (one strip) or Ws + 2 (strips) for planes from 2 columns up to the widest strip the halo buffers admit,
    # and beyond; wave columns 0 .. 3 (4-wave kind) and 0 .. 7 (128 x 512 units)
    worst = {}
    for pitch in range(3, 260):
        for tap in range(9):
            for wn in range(8):
                c = plan(b"sk_halo_cycles", pitch, tap, wn, 0.0)
                if c != 4:
                    worst[(pitch, tap, wn)] = c
    assert not worst, sorted(worst.items())[:16]


def test_halo_cycles_query_rejects_bad_arguments():
    plan = ulib.load().ucdir_debug_launch_plan
    assert plan(b"sk_halo_cycles", 0, 0, 0, 0.0) == -1
    assert plan(b"sk_halo_cycles", 19, 9, 0, 0.0) == -1
    assert plan(b"sk_halo_cycles", 19, 0, 8, 0.0) == -1
