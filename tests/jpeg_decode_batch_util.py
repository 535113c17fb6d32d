"""Shared by tests/test_jpeg_decode_batch_cpu.py and tests/test_jpeg_decode_batch_gpu.py: the host side of a batch decode
(csrc/jpeg_decode.hip.h, "several files per call") through the C interface, and the descriptor table read back with numpy."""
import numpy as np

import jpeg_decode_model as D
from ucdir_amd import lib

HEADER_U32 = ("magic", "n", "nitems", "idct_wgs", "colour_wgs", "reserved")
HEADER_U64 = ("off_items", "off_idct", "off_colour", "table_bytes", "ws_bytes", "zero_bytes", "out_bytes", "buffer_bytes")
FILE_U64 = ("packed_off", "out_off", "coef_off", "state_off", "first_off", "rounds_off", "planes_off")
FILE_I32 = ("packed_len", "nseg", "nsub", "nmcu", "bpm", "nluma", "restart", "nblk", "W", "H", "ncomp", "hs", "vs", "mcus_x", "x0", "y0", "w", "h")
MAGIC = 0x3142444a


def up16(v):
    return (v + 15) // 16 * 16


def infos_of(datas):
    """The info words of every file, by ucdir_jpeg_decode_info (tests/test_jpeg_decode_cpu.py holds it to the model's parse)."""
    L = lib.load()
    out = np.zeros((len(datas), 16), np.int32)
    for k, d in enumerate(datas):
        src = np.frombuffer(d, np.uint8)
        assert L.ucdir_jpeg_decode_info(src.ctypes.data, len(d), out[k].ctypes.data) == 0, k
    return out


def pack(data, info):
    """The packed stream, by ucdir_jpeg_decode_pack (held to the model's pack there too)."""
    src, out = np.frombuffer(data, np.uint8), np.zeros(int(info[9]), np.uint8)
    assert lib.load().ucdir_jpeg_decode_pack(src.ctypes.data, len(data), out.ctypes.data, len(out)) == len(out)
    return out.tobytes()


def query(infos):
    """(table bytes, workspace bytes) of the query form; table bytes is -1 on a refusal."""
    ws = np.full(1, -1, np.int64)
    infos = np.ascontiguousarray(infos, np.int32)
    n = lib.load().ucdir_jpeg_decode_batch_plan(len(infos), infos.ctypes.data, None, None, None, None, 0, ws.ctypes.data)
    return n, int(ws[0])


class Batch:
    """The host buffer of a batch (table, then the packed streams at 16-byte aligned offsets, ``gap`` spare bytes between them) and
    what the plan answered.  ``rc``: the plan's return value; the table is only read when it is positive."""

    def __init__(self, datas, crops=None, gap=0, infos=None, packed_off=None, out_off=None, cap=None):
        L = lib.load()
        self.datas = list(datas)
        self.n = len(self.datas)
        true = infos_of(self.datas)
        self.infos = true if infos is None else np.ascontiguousarray(infos, np.int32)
        self.packed = [pack(d, i) for d, i in zip(self.datas, true)]
        self.table_bytes, self.ws_bytes = query(true)
        assert self.table_bytes > 0
        whole = [(0, 0, int(i[0]), int(i[1])) for i in true]
        self.crops = [c if c is not None else w for c, w in zip(crops or [None] * self.n, whole)]
        sizes = [up16(len(p)) + 16 * gap for p in self.packed]
        self.packed_off = np.array(self.table_bytes + np.concatenate([[0], np.cumsum(sizes)[:-1]]), np.int64) if packed_off is None else np.array(packed_off, np.int64)
        self.out_sizes = [3 * c[2] * c[3] for c in self.crops]
        self.out_off = np.array(np.concatenate([[0], np.cumsum(self.out_sizes)[:-1]]), np.int64) if out_off is None else np.array(out_off, np.int64)
        total = self.table_bytes + sum(sizes)
        self.buf = np.full(total, 0xA5, np.uint8)
        for p, o in zip(self.packed, self.table_bytes + np.concatenate([[0], np.cumsum(sizes)[:-1]])):
            self.buf[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
        before = self.buf.copy()
        crop_arr = np.array(self.crops, np.int32)
        self.rc = L.ucdir_jpeg_decode_batch_plan(self.n, self.infos.ctypes.data, crop_arr.ctypes.data if crops is not None else None,
                                                 self.packed_off.ctypes.data, self.out_off.ctypes.data, self.buf.ctypes.data,
                                                 total if cap is None else cap, None)
        self.error = L.ucdir_last_error().decode() if self.rc < 0 else ""
        if self.rc < 0:
            assert np.array_equal(self.buf, before)                   # a refusal writes nothing
        else:
            assert np.array_equal(self.buf[self.table_bytes:], before[self.table_bytes:])

    def table(self):
        """The table as a dict: the header's fields, "files" (a list of dicts), "items" (nitems x 2), "idct" and "colour" (n + 1)."""
        b = self.buf
        t = dict(zip(HEADER_U32, b[:24].view(np.uint32).tolist()))
        t.update(zip(HEADER_U64, b[24:88].view(np.uint64).tolist()))
        assert not b[88:128].any()
        n = t["n"]
        t["files"] = []
        for k in range(n):
            r = b[128 + 128 * k:256 + 128 * k]
            f = dict(zip(FILE_U64, r[:56].view(np.uint64).tolist()))
            f.update(zip(FILE_I32, r[56:128].view(np.int32).tolist()))
            t["files"].append(f)
        t["items"] = b[t["off_items"]:t["off_items"] + 8 * t["nitems"]].view(np.uint32).reshape(-1, 2).astype(np.int64)
        t["idct"] = b[t["off_idct"]:t["off_idct"] + 4 * (n + 1)].view(np.uint32).astype(np.int64)
        t["colour"] = b[t["off_colour"]:t["off_colour"] + 4 * (n + 1)].view(np.uint32).astype(np.int64)
        return t


def segment_bits(packed, nseg):
    """Bit length of every restart segment, from the packed stream's segment table."""
    return np.frombuffer(packed, np.uint32, 4 * nseg, D.OFF_SEG).reshape(nseg, 4)[:, 1].astype(np.int64)
