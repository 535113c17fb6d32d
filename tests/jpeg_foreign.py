"""A baseline JPEG writer for tests, and the catalogue of files it writes: files as encoders other than libjpeg write them, which the
decoder (csrc/jpeg_decode.hip.h) has to take all the same.  Every file written by Pillow or by the project's own encoder has a JFIF
marker, component ids 1 2 3, quantisation tables 0 and 1, Huffman tables 0 for luma and 1 for chroma, the Annex K tables or
libjpeg's optimised ones, one table per segment, 1-bit padding and nothing between the last MCU and the next marker; write() below
varies each of these habits on its own.

The coefficients are those of real pixels: a float64 forward DCT, divided by the chosen tables and rounded, so every file is an
encoding an encoder could have produced (write() asserts the baseline categories and that dequantised values stay far from 16
bits).  write() returns the bytes and the pixels tests/jpeg_decode_model.py's reconstruct makes of the same coefficients, without
parsing the file again: Pillow equal to those pixels says that the writer wrote what it meant to.

catalogue() names the files and what each must show; tests/test_jpeg_foreign_cpu.py holds Pillow, the model and the library's host
functions to it, tests/test_jpeg_foreign_gpu.py the kernels."""
import collections
import functools
import struct

import numpy as np

import jpeg_decode_model as D
import jpeg_encode_model as E
from jpeg_encode_model import ZIGZAG, huff_codes, make_content

_K = np.arange(8)
_C = np.cos((2 * _K[None, :] + 1) * _K[:, None] * np.pi / 16) / 2            # F = C X C^T: the DCT of T.81 A.3.3
_C[0] /= np.sqrt(2)
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "L": (1, 1)}
DC_SYMBOLS = list(range(12))
AC_SYMBOLS = [0x00, 0xf0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
S_BYTES = D.S // 8


# ---- quantisation tables (64 entries, natural order) -----------------------------------------------------------------------------
def qtable(kind):
    if kind == "luma90":
        return E.quant_table(E.STD_LUMA, 90).ravel()
    if kind == "chroma90":
        return E.quant_table(E.STD_CHROMA, 90).ravel()
    if kind == "chroma75":
        return E.quant_table(E.STD_CHROMA, 75).ravel()
    if kind == "ones":
        return np.ones(64, np.int64)
    if kind == "to255":                                   # quality 90 in front, 255 from zigzag position 10 on
        q = E.quant_table(E.STD_LUMA, 90).ravel().copy()
        q[ZIGZAG[10:]] = 255
        return q
    raise ValueError(kind)


# ---- Huffman tables: (bits[16], vals) ---------------------------------------------------------------------------------------------
def annex_k(cls, tid):
    return (list(E.DC_BITS[tid]), list(E.DC_VALS)) if cls == 0 else (list(E.AC_BITS[tid]), list(E.AC_VALS[tid]))


def _by_frequency(cls, freq, reverse):
    syms = DC_SYMBOLS if cls == 0 else AC_SYMBOLS
    return sorted(syms, key=lambda s: (freq.get(s, 0) if reverse else -freq.get(s, 0), s))


def unary_table(cls, freq, reverse=False):
    """Every symbol of the class, the most frequent first (reverse: last): lengths 1, 2, 3 ... for as many symbols as leave room
    for the rest at 16 bits - twelve DC symbols take 1 .. 12, the 162 AC symbols 1 .. 8 and 154 codes of 16 bits."""
    vals = _by_frequency(cls, freq, reverse)
    k = max(k for k in range(1, 16) if len(vals) - k <= (1 << (16 - k)) - 1 and k <= len(vals))
    bits = [1] * k + [0] * (15 - k) + [len(vals) - k]
    return bits, vals


def long_dc_table(freq):
    """A DC table without a code of 8 bits or less: four codes of 9, four of 12 and four of 16 bits, the most frequent first."""
    bits = [0] * 16
    bits[8] = bits[11] = bits[15] = 4
    return bits, _by_frequency(0, freq, False)


def make_table(spec, cls, tid, freq):
    if spec == "annexk":
        return annex_k(cls, tid)
    if spec == "annexk-other":                            # the other id's Annex K table: a decoy, or a table that is never used
        return annex_k(cls, 1 - tid)
    if spec == "unary":
        return unary_table(cls, freq)
    if spec == "reversed":
        return unary_table(cls, freq, reverse=True)
    if spec == "longdc":
        assert cls == 0
        return long_dc_table(freq)
    bits, vals = spec
    return list(bits), list(vals)


# ---- pixels -> quantised coefficients ---------------------------------------------------------------------------------------------
def coefficients(img, sampling, qts, rgb=False):
    """(blocks (n, 64) int64 in natural order and scan order, component of every block, geometry dict).  qts: the table of every
    component.  Chroma is box-averaged; every plane is padded to whole MCUs by replicating its edge."""
    a = img.astype(np.float64)
    R, G, B = a[..., 0], a[..., 1], a[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    if sampling == "L":
        comps = [Y]
    elif rgb:
        comps = [R, G, B]
    else:
        comps = [Y, 128 - 0.168736 * R - 0.331264 * G + 0.5 * B, 128 + 0.5 * R - 0.418688 * G - 0.081312 * B]
    hs, vs = SAMPLINGS[sampling]
    H, W = img.shape[:2]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    per = []
    for c, p in enumerate(comps):
        p = np.pad(p, ((0, my * 8 * vs - H), (0, mx * 8 * hs - W)), mode="edge")
        if c > 0:
            p = p.reshape(my * 8, vs, mx * 8, hs).mean(axis=(1, 3))
        x = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2) - 128
        f = _C @ x @ _C.T
        q = np.rint(f / np.asarray(qts[c], np.float64).reshape(8, 8)).astype(np.int64)
        assert np.abs(q * np.asarray(qts[c]).reshape(8, 8)).max() < 16384
        per.append(q.reshape(q.shape[0], q.shape[1], 64))
    luma = per[0].reshape(my, vs, mx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, vs * hs, 64)
    mcus = np.concatenate([luma] + [p[:, :, None, :] for p in per[1:]], axis=2)
    bpm = mcus.shape[2]
    comp = [0] * (vs * hs) + list(range(1, len(comps)))
    geo = dict(width=W, height=H, components=len(comps), h_samp=hs, v_samp=vs, blocks_per_mcu=bpm, mcus_x=mx, mcus_y=my)
    return mcus.reshape(-1, 64), comp, geo


def expected_pixels(blocks, geo, qts, rgb=False):
    """reconstruct() of the coefficients write() was given; an RGB-coded file is three greyscale planes."""
    def P(g, tables):
        return dict(info=g, quant={c: np.asarray(t, np.uint8) for c, t in enumerate(tables)}, sel=np.array([0, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0]))
    if not rgb:
        return D.reconstruct(P(geo, qts), blocks)
    assert geo["blocks_per_mcu"] == 3 and geo["h_samp"] == geo["v_samp"] == 1
    grey = dict(geo, components=1, blocks_per_mcu=1)
    return np.stack([D.reconstruct(P(grey, [qts[c]]), blocks[c::3])[..., 0] for c in range(3)], -1)


# ---- coefficients -> symbols -> bits ----------------------------------------------------------------------------------------------
def _nbits(v):
    return int(abs(int(v))).bit_length()


def scan_symbols(blocks, comp, restart):
    """Per restart segment, the symbols of its blocks in order: (component, class, symbol, magnitude bits, their count)."""
    bpm, nmcu = len(comp), len(blocks) // len(comp)
    per = restart if restart else nmcu
    segs = []
    for m0 in range(0, nmcu, per):
        out, last = [], {}
        for g in range(m0 * bpm, min(m0 + per, nmcu) * bpm):
            c, zz = comp[g % bpm], blocks[g][ZIGZAG]
            diff = int(zz[0]) - last.get(c, 0)
            last[c] = int(zz[0])
            s = _nbits(diff)
            assert s <= 11, diff
            out.append((c, 0, s, (diff - 1 if diff < 0 else diff) & ((1 << s) - 1), s))
            prev = 0
            nz = np.flatnonzero(zz[1:]) + 1
            for k in nz:
                v, r = int(zz[k]), int(k) - prev - 1
                prev = int(k)
                while r > 15:
                    out.append((c, 1, 0xf0, 0, 0))
                    r -= 16
                s = _nbits(v)
                assert s <= 10, v
                out.append((c, 1, (r << 4) | s, (v - 1 if v < 0 else v) & ((1 << s) - 1), s))
            if len(nz) == 0 or nz[-1] != 63:
                out.append((c, 1, 0x00, 0, 0))
        segs.append(out)
    return segs


def _bits_of(vals, lens):
    pos = np.concatenate([[0], np.cumsum(lens)])
    bits = np.zeros(int(pos[-1]), np.uint8)
    for t in range(int(lens.max())):
        m = lens > t
        bits[pos[:-1][m] + t] = (vals[m] >> (lens[m] - 1 - t)) & 1
    return bits, pos


def _stuff(raw):
    raw = np.frombuffer(raw, np.uint8)
    return np.insert(raw, np.flatnonzero(raw == 0xff) + 1, 0).tobytes()


# ---- the file --------------------------------------------------------------------------------------------------------------------
File = collections.namedtuple("File", "data pixels meta")


def write(img, sampling="444", quant=("luma90", "chroma90", "chroma90"), quant_ids=(0, 1, 1), tables=None, dc_sel=(0, 1, 1),
          ac_sel=(0, 1, 1), restart=0, dri=None, dri_early=None, order=("dqt", "sof", "dht", "dri"), merge_dht=False, merge_dqt=False,
          redefine=(), extra_dqt=(), extra_dht=(), app=("jfif",), comp_ids=(1, 2, 3), grey_sampling=(1, 1), rgb=False, fill=0,
          trailing=b"", eoi=True, pad="ones", spare=b"", spare_where="last", seed=0):
    """The bytes of a baseline file of ``img`` (H, W, 3 uint8), its expected pixels and a dict about it.

    sampling      "444", "422", "420" or "L" (greyscale; grey_sampling: the factors its SOF declares)
    quant         the table of every component (a qtable() name or 64 entries in natural order); quant_ids: its id, 0 .. 3.
                  Components that share an id must share the table
    tables        {(class, id): "annexk" | "unary" | "reversed" | "longdc" | (bits, vals)} for the slots the components use
                  (default: Annex K); dc_sel / ac_sel: the id every component's DC / AC codes come from
    restart       MCUs per restart segment, 0: none.  dri: the values of the DRI segments at the "dri" place of ``order`` (default:
                  [restart], nothing for 0); the last one must say how the scan is cut.  dri_early: one more, in front of all tables
    order         "dqt", "sof", "dht", "dri" in the order of their segments; SOS is last
    merge_dht / merge_dqt   all tables of the kind in one segment
    redefine      ("dqt", id) / ("dht", class, id): a different definition in front of the one that counts (in the same segment
                  when merged)
    extra_dqt / extra_dht   ids / (class, id) slots of tables nothing uses
    app           in order: "jfif", ("adobe", transform), ("app1_jpeg", bytes), ("app2_chain", n), "com"
    comp_ids      the ids of SOF and SOS.  rgb: the three components are R, G, B themselves (4:4:4 only)
    fill          FF bytes in front of every marker behind SOI, RSTn and EOI included: a count, or "seeded" for 1 .. 3 each
    trailing      bytes behind EOI; eoi=False: no EOI
    pad           the bits that fill every segment's last byte: "ones", "zeros", "random", or a string of 0 and 1 that is repeated
    spare         whole bytes behind the padding of the last segment (spare_where="all": of every segment), stuffed like the rest"""
    rs = np.random.RandomState(seed)
    nc = 1 if sampling == "L" else 3
    qts = [qtable(q) if isinstance(q, str) else np.asarray(q, np.int64) for q in quant[:nc]]
    for c in range(nc):
        for d in range(c):
            assert quant_ids[c] != quant_ids[d] or np.array_equal(qts[c], qts[d])
        assert qts[c].min() >= 1 and qts[c].max() <= 255
    blocks, comp, geo = coefficients(img, sampling, qts, rgb)
    H, W, bpm = geo["height"], geo["width"], geo["blocks_per_mcu"]
    nmcu = geo["mcus_x"] * geo["mcus_y"]
    dri = list(dri) if dri is not None else ([restart] if restart else [])
    declared = dri[-1] if dri else (dri_early or 0)
    assert (declared if declared < nmcu else 0) == (restart if restart < nmcu else 0), "the last DRI must say how the scan is cut"
    segs = scan_symbols(blocks, comp, restart)

    # Huffman tables: the slots in use, built from the symbols of the components that use them
    tables = dict(tables or {})
    freq = collections.defaultdict(collections.Counter)
    for out in segs:
        for c, cls, sym, _, _ in out:
            freq[(cls, (ac_sel if cls else dc_sel)[c])][sym] += 1
    used = sorted(freq)
    built = {slot: make_table(tables.get(slot, "annexk"), slot[0], slot[1], freq[slot]) for slot in used}
    codes = {slot: huff_codes(*t) for slot, t in built.items()}

    # the entropy-coded bytes
    scan, seg_bytes, symbol_bits = bytearray(), [], []
    for k, out in enumerate(segs):
        cl = [codes[(cls, (ac_sel if cls else dc_sel)[c])][sym] for c, cls, sym, _, _ in out]
        lens = np.array([l + s for (_, l), (_, _, _, _, s) in zip(cl, out)], np.int64)
        vals = np.array([(code << s) | mag for (code, _), (_, _, _, mag, s) in zip(cl, out)], np.int64)
        bits, pos = _bits_of(vals, lens)
        n = -len(bits) % 8
        if pad == "ones":
            tail = np.ones(n, np.uint8)
        elif pad == "zeros":
            tail = np.zeros(n, np.uint8)
        elif pad == "random":
            tail = rs.randint(0, 2, n).astype(np.uint8)
        else:
            tail = np.array([int(ch) for ch in (pad * 8)[:n]], np.uint8)
        raw = np.packbits(np.concatenate([bits, tail])).tobytes()
        if spare and (spare_where == "all" or k == len(segs) - 1):
            raw += spare
        seg_bytes.append(len(raw))
        symbol_bits.append(pos)
        if k:
            scan += b"\xff" * (rs.randint(1, 4) if fill == "seeded" else fill) + bytes([0xff, 0xd0 + (k - 1) % 8])
        scan += _stuff(raw)

    # the segments in front of the scan
    pieces = []

    def seg(marker, payload):
        assert len(payload) + 2 <= 65535
        pieces.append(bytes([0xff, marker]) + struct.pack(">H", len(payload) + 2) + payload)

    for a in app:
        if a == "jfif":
            seg(0xe0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
        elif a == "com":
            seg(0xfe, b"written by tests/jpeg_foreign.py \xff\xd9 \xff\xda")
        elif a[0] == "adobe":
            seg(0xee, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([a[1]]))
        elif a[0] == "app1_jpeg":
            seg(0xe1, b"Thumb\x00" + a[1])
        elif a[0] == "app2_chain":                        # maximal segments of seeded bytes: markers inside them are payload
            for _ in range(a[1]):
                seg(0xe2, b"chain\x00" + rs.randint(0, 256, 65533 - 6).astype(np.uint8).tobytes())
        else:
            raise ValueError(a)
    if dri_early is not None:
        seg(0xdd, struct.pack(">H", dri_early))

    def dqt(tid, q):
        return bytes([tid]) + bytes(np.asarray(q, np.int64)[ZIGZAG].tolist())

    def dht(slot, t):
        return bytes([(slot[0] << 4) | slot[1]]) + bytes(t[0]) + bytes(t[1])

    for what in order:
        if what == "dqt":
            parts = []
            for tid in sorted(set(quant_ids[:nc]) | set(extra_dqt)):
                if ("dqt", tid) in redefine:
                    parts.append(dqt(tid, np.full(64, 7)))
                parts.append(dqt(tid, qts[quant_ids.index(tid)] if tid in quant_ids[:nc] else np.arange(1, 65)))
            for p in ([b"".join(parts)] if merge_dqt else parts):
                seg(0xdb, p)
        elif what == "dht":
            parts = []
            for slot in sorted(set(used) | set(extra_dht)):
                if ("dht",) + slot in redefine:           # a decoy: the other kind of table for the same slot
                    parts.append(dht(slot, make_table("unary" if tables.get(slot, "annexk") == "annexk" else "annexk", slot[0], slot[1], {})))
                parts.append(dht(slot, built[slot] if slot in built else make_table("annexk-other", slot[0], slot[1], {})))
            for p in ([b"".join(parts)] if merge_dht else parts):
                seg(0xc4, p)
        elif what == "dri":
            for v in dri:
                seg(0xdd, struct.pack(">H", v))
        elif what == "sof":
            body = bytes([8, H >> 8, H & 255, W >> 8, W & 255, nc])
            for c in range(nc):
                h, v = (grey_sampling if nc == 1 else (geo["h_samp"], geo["v_samp"]) if c == 0 else (1, 1))
                body += bytes([comp_ids[c], (h << 4) | v, quant_ids[c]])
            seg(0xc0, body)
        else:
            raise ValueError(what)
    seg(0xda, bytes([nc]) + b"".join(bytes([comp_ids[c], (dc_sel[c] << 4) | ac_sel[c]]) for c in range(nc)) + b"\x00\x3f\x00")

    def filled(piece):
        return b"\xff" * (rs.randint(1, 4) if fill == "seeded" else fill) + piece

    data = b"\xff\xd8" + b"".join(filled(p) for p in pieces) + bytes(scan)
    if eoi:
        data += filled(b"\xff\xd9")
    data += trailing
    meta = dict(geo, mcus=nmcu, segment_bytes=seg_bytes, symbol_bits=symbol_bits, tables=built, header_bytes=len(data) - len(scan))
    return File(data, expected_pixels(blocks, geo, qts, rgb), meta)


# ---- the seeded searches ----------------------------------------------------------------------------------------------------------
GRID_CONTENT, GRID_RESTART = ("noise", 40, 56), 15       # 35 MCUs in 4:4:4 of about 119.5 bytes: 15 of them fill 14 subsequences


@functools.lru_cache(maxsize=None)
def grid_seeds():
    """{residue: (seed, segment)} for 0, 1 and 127: the first noise seed whose 4:4:4 file with restart interval 15 has a segment of
    at least two subsequences whose unstuffed length is that residue modulo the 128 bytes of a subsequence."""
    found = {}
    for seed in range(400):
        lens = write(make_content(*GRID_CONTENT, seed), restart=GRID_RESTART).meta["segment_bytes"]
        for k, n in enumerate(lens):
            if n > S_BYTES and n % S_BYTES in (0, 1, S_BYTES - 1):
                found.setdefault(n % S_BYTES, (seed, k))
        if len(found) == 3:
            return found
    raise AssertionError("no seed below 400")


@functools.lru_cache(maxsize=None)
def extreme_seed():
    """The first noise seed whose 33 x 15 4:4:4 file (one segment) has a symbol that begins on the last bit of a subsequence and
    another that ends exactly where a subsequence ends, both in front of the last subsequence."""
    for seed in range(400):
        f = write(make_content("noise", 33, 15, seed))
        pos = f.meta["symbol_bits"][0]
        inner = pos[pos < (f.meta["segment_bytes"][0] * 8 // D.S) * D.S + 1]
        if (inner[:-1] % D.S == D.S - 1).any() and (inner[1:] % D.S == 0).any():
            return seed
    raise AssertionError("no seed below 400")


@functools.lru_cache(maxsize=None)
def never_synchronising_side():
    """The smallest square noise image whose 4:4:4 file with reversed tables, one pair for all three components, has more than
    256 subsequences in its one segment."""
    for side in range(64, 129):
        f = never_synchronising(side)
        if -(-f.meta["segment_bytes"][0] // S_BYTES) > 256:
            return side
    raise AssertionError("no side below 129")


def never_synchronising(side, **kw):
    return write(make_content("noise", side, side), tables={(0, 0): "reversed", (1, 0): "reversed"}, dc_sel=(0, 0, 0), ac_sel=(0, 0, 0), **kw)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
Entry = collections.namedtuple("Entry", "name data pixels meta shows check")
Seen = collections.namedtuple("Seen", "data meta P st status symbols padding_not_ones")    # what a check is given, by seen()

SPARE_BYTES, NO_EOI, RGB_CODED = "spare whole bytes between the last MCU and the marker", "no EOI", "RGB-coded"
# the files that stay refused: name -> (class, code of host, model and device; 1000 + the status bits for the kernels' refusals).
# The status of the spare bytes: 00 00 decodes as codes of the Annex K tables, each of them a write past the segment's last block
# (ST_WRITE), none of them a complete block; a spare FF behind 1-bit padding is a run of 1-bits that matches no DC code
# (ST_NO_CODE) and is such a write too; 001010 and a spare 00101000 behind flat blocks are two complete blocks of 6 bits more than
# the segment has (ST_BLOCK_TOTAL as well).
MUST_REFUSE = {
    "spare 00 00 before EOI": (SPARE_BYTES, 1000 + D.ST_WRITE),
    "spare FF before EOI": (SPARE_BYTES, 1000 + D.ST_WRITE + D.ST_NO_CODE),
    "spare 00 before every RSTn, 4:2:0": (SPARE_BYTES, 1000 + D.ST_WRITE),
    "zero padding and a spare 00": (SPARE_BYTES, 1000 + D.ST_WRITE),
    "flat greyscale, whole spare blocks": (SPARE_BYTES, 1000 + D.ST_WRITE + D.ST_BLOCK_TOTAL),
    "no EOI": (NO_EOI, D.BAD_NO_EOI),
    "no EOI, zero padding, restart markers": (NO_EOI, D.BAD_NO_EOI),
    "ids R G B without a marker": (RGB_CODED, D.UNSUP_COLOUR),
    "Adobe transform 0": (RGB_CODED, D.UNSUP_COLOUR),
}
PILLOW_REFUSES = (NO_EOI,)                                 # Image.load raises for these; the other two classes it decodes


def _info(s, **want):
    return all(s.P["info"][k] == v for k, v in want.items())


def _sel(s):
    return [tuple(int(v) for v in s.P["sel"][4 * c:4 * c + 3]) for c in range(s.P["info"]["components"])]


def _count(s, marker):
    """Segments with this marker in front of the scan, by a walk of the lengths."""
    pos, n = 2, 0
    while True:
        if s.data[pos + 1] == 0xff:
            pos += 1
            continue
        n += s.data[pos + 1] == marker
        if s.data[pos + 1] == 0xda:
            return n
        pos += 2 + ((s.data[pos + 2] << 8) | s.data[pos + 3])


def _place(s, marker):
    return s.data.index(bytes([0xff, marker]))


@functools.lru_cache(maxsize=None)
def catalogue():
    out = []

    def add(name, shows, check, content=("noise", 40, 56, 0), f=None, **kw):
        f = f if f is not None else write(make_content(*content), **kw)
        assert name not in [e.name for e in out]
        out.append(Entry(name, f.data, f.pixels, f.meta, shows, check))

    small, odd = ("noise", 7, 9, 0), ("real", 33, 15, 0)
    one = dict(dc_sel=(0, 0, 0), ac_sel=(0, 0, 0))
    # Huffman tables
    add("Annex K, JFIF, ids 1 2 3", "the habits of libjpeg, by this writer", lambda s: _info(s, segments=1, blocks=105) and _sel(s) == [(0, 0, 2), (1, 1, 3), (1, 1, 3)])
    add("unary tables", "frequency-sorted codes of 1, 2, 3 ... bits, the rest 16", lambda s: s.st["max_ac_code"] == 16 and sum(s.P["huff"][2][0][:8]) == 8,
        tables={k: "unary" for k in ((0, 0), (0, 1), (1, 0), (1, 1))})
    add("reversed tables", "the frequent symbols take the 16-bit codes", lambda s: s.st["max_ac_code"] == 16 and s.st["max_dc_code"] > 8 and s.st["rounds"] > 8,
        tables={k: "reversed" for k in ((0, 0), (0, 1), (1, 0), (1, 1))})
    add("long DC codes", "every DC code in use is longer than 8 bits", lambda s: s.st["max_dc_code"] > 8 and min(l for slot in (0, 1) for l, n in enumerate(s.P["huff"][slot][0], 1) if n) == 9,
        tables={(0, 0): "longdc", (0, 1): "longdc"})
    add("long DC codes, 4:2:0, 33x15", "the same behind four luma blocks per MCU", lambda s: s.st["max_dc_code"] > 8 and _info(s, blocks_per_mcu=6),
        content=odd, sampling="420", tables={(0, 0): "longdc", (0, 1): "longdc"})
    # which table id each component uses
    add("luma on 1, chroma on 0", "Huffman ids swapped", lambda s: _sel(s) == [(0, 1, 3), (1, 0, 2), (1, 0, 2)], dc_sel=(1, 0, 0), ac_sel=(1, 0, 0))
    add("one table pair for all", "every component on DC 0 / AC 0: never synchronising, as many rounds as subsequences",
        lambda s: _sel(s) == [(0, 0, 2), (1, 0, 2), (1, 0, 2)] and sorted(s.P["huff"]) == [0, 2] and s.st["rounds"] == s.st["subsequences"] > 30, **one)
    add("a different mix per component", "DC and AC ids differ inside a component and between all three",
        lambda s: _sel(s) == [(0, 0, 3), (1, 1, 3), (1, 1, 2)], dc_sel=(0, 1, 1), ac_sel=(1, 1, 0), tables={(1, 0): "unary", (0, 1): "unary"})
    add("a different mix per component, 4:2:0", "the selectors behind four luma blocks", lambda s: _sel(s) == [(0, 1, 2), (1, 0, 2), (1, 1, 3)] and _info(s, blocks_per_mcu=6),
        sampling="420", dc_sel=(1, 0, 1), ac_sel=(0, 0, 1))
    # quantisation
    add("quantisation ids 2 and 3", "tables 0 and 1 never defined", lambda s: sorted(s.P["quant"]) == [2, 3] and [t[0] for t in _sel(s)] == [2, 3, 3], quant_ids=(2, 3, 3))
    add("three quantisation tables", "Cb and Cr on different tables", lambda s: [t[0] for t in _sel(s)] == [3, 0, 2] and len({s.P["quant"][k].tobytes() for k in (0, 2, 3)}) == 3,
        quant=("luma90", "chroma90", "chroma75"), quant_ids=(3, 0, 2))
    add("quantisation entries of 1", "a table of ones", lambda s: set(s.P["quant"][0].tolist()) == {1}, content=("real", 40, 56, 0), quant=("ones", "chroma90", "chroma90"))
    add("quantisation entries of 255", "255 from zigzag position 10 on, and a table of ones for Cr", lambda s: int(s.P["quant"][1].max()) == 255 and set(s.P["quant"][2].tolist()) == {1},
        quant=("luma90", "to255", "ones"), quant_ids=(0, 1, 2))
    # segment layout
    add("every DHT in one segment", "four tables behind one marker", lambda s: _count(s, 0xc4) == 1 and sorted(s.P["huff"]) == [0, 1, 2, 3], merge_dht=True)
    add("every DQT in one segment", "two tables behind one marker", lambda s: _count(s, 0xdb) == 1 and sorted(s.P["quant"]) == [0, 1], merge_dqt=True)
    add("tables in front of SOF", "DQT and DHT, then SOF", lambda s: max(_place(s, 0xdb), _place(s, 0xc4)) < _place(s, 0xc0), order=("dqt", "dht", "dri", "sof"), restart=4)
    add("tables behind SOF", "SOF, then DQT and DHT", lambda s: _place(s, 0xc0) < min(_place(s, 0xdb), _place(s, 0xc4)), order=("sof", "dht", "dqt"))
    add("tables defined twice", "a decoy definition of two Huffman tables and a quantisation table in front of the real ones",
        lambda s: _count(s, 0xc4) == 6 and _count(s, 0xdb) == 3 and s.P["huff"][2] == tuple(annex_k(1, 0)) and int(s.P["quant"][1][0]) != 7,
        redefine=(("dht", 1, 0), ("dht", 0, 1), ("dqt", 1)))
    add("tables defined twice in one segment", "the decoys and the real tables behind one marker each", lambda s: _count(s, 0xc4) == 1 and _count(s, 0xdb) == 1 and int(s.P["quant"][0][0]) != 7,
        redefine=(("dht", 1, 1), ("dht", 0, 0), ("dqt", 0)), merge_dht=True, merge_dqt=True, tables={(1, 1): "unary"})
    add("unused extra tables", "a quantisation table 3 and Huffman tables 1 that nothing uses", lambda s: sorted(s.P["quant"]) == [0, 1, 3] and sorted(s.P["huff"]) == [0, 1, 2, 3] and {t[1:] for t in _sel(s)} == {(0, 2)},
        extra_dqt=(3,), extra_dht=((0, 1), (1, 1)), **one)
    add("DRI in front of everything", "DRI, then the tables", lambda s: _place(s, 0xdd) < _place(s, 0xdb) and _info(s, restart_interval=5, segments=7), restart=5, dri=[], dri_early=5)
    add("DRI 0", "a DRI segment that switches restarts off", lambda s: _count(s, 0xdd) == 1 and _info(s, restart_interval=0, segments=1), dri=[0])
    add("DRI larger than the MCU count", "65535 for 35 MCUs: one segment", lambda s: _info(s, restart_interval=65535, segments=1), restart=65535)
    add("DRI given twice", "the second one counts", lambda s: _count(s, 0xdd) == 2 and _info(s, restart_interval=4, segments=9), restart=4, dri=[4], dri_early=7)
    add("DRI switched off again", "DRI 9, then DRI 0", lambda s: _count(s, 0xdd) == 2 and _info(s, restart_interval=0, segments=1), dri=[9, 0])
    # markers
    add("Adobe transform 1, no JFIF", "YCbCr by the Adobe marker", lambda s: _count(s, 0xee) == 1 and _count(s, 0xe0) == 0, app=(("adobe", 1),))
    add("Adobe transform 0 behind JFIF", "JFIF decides: YCbCr", lambda s: _count(s, 0xee) == 1 and _count(s, 0xe0) == 1, app=("jfif", ("adobe", 0)))
    add("Adobe transform 0", "RGB by the Adobe marker", lambda s: s.P is None and _count(s, 0xee) == 1 and _count(s, 0xe0) == 0,
        content=odd, app=(("adobe", 0),), rgb=True)
    for ids, label in (((1, 2, 3), "1 2 3"), ((0, 1, 2), "0 1 2"), ((ord("Y"), ord("C"), ord("c")), "Y C c")):
        add(f"ids {label} without a marker", "YCbCr by the component ids", lambda s: _count(s, 0xe0) + _count(s, 0xee) == 0 and _info(s, components=3),
            content=odd, app=(), comp_ids=ids)
    add("ids R G B without a marker", "RGB by the component ids", lambda s: s.P is None and bytes([3, ord("R"), 0, ord("G"), 0x11, ord("B"), 0x11]) in s.data,
        content=odd, app=(), comp_ids=(ord("R"), ord("G"), ord("B")), rgb=True)
    thumb = write(make_content("real", 16, 16), sampling="420").data
    add("a whole JPEG inside APP1", "SOI ... EOI of another file as payload", lambda s: s.data.count(b"\xff\xd8") == 2 and s.data.count(b"\xff\xc0") == 2 and _info(s, width=9, height=7),
        content=small, app=("jfif", ("app1_jpeg", thumb)))
    add("a chain of maximal APP2 segments", "three segments of 65535 bytes of seeded bytes", lambda s: _count(s, 0xe2) == 3 and s.P["scan"][0] > 3 * 65537 and _info(s, width=9, height=7),
        content=small, app=("jfif", ("app2_chain", 3)))
    add("COM", "a comment that holds EOI and SOS", lambda s: _count(s, 0xfe) == 1, content=small, app=("com", "jfif"))
    add("fill bytes in front of every marker", "1 to 3 FF in front of each, RSTn and EOI included",
        lambda s: _info(s, segments=18) and all(bytes([0xff, 0xff, m]) in s.data for m in (0xe0, 0xdb, 0xc0, 0xc4, 0xdd, 0xda, 0xd9) + tuple(range(0xd0, 0xd8))),
        fill="seeded", restart=2, seed=3)
    add("three fill bytes everywhere, 4:2:0", "FF FF FF in front of each marker", lambda s: s.data.count(b"\xff\xff\xff\xff") >= 9 + 11 and _info(s, segments=12), sampling="420", fill=3, restart=1)
    add("bytes after EOI", "another SOI and zeros behind the end", lambda s: not s.data.endswith(b"\xff\xd9") and s.data[s.P["scan"][1]:s.P["scan"][1] + 2] == b"\xff\xd9", trailing=b"\xff\xd8\x00\x00\xff\xd9\x00")
    # sampling and sizes
    for smp in ("444", "422", "420", "L"):
        for content in (small, odd, ("real", 40, 56, 0)):
            hs, vs = SAMPLINGS[smp]
            add(f"{smp} {content[1]}x{content[2]}", "a sampling at a size", lambda s, smp=smp, hs=hs, vs=vs, c=content: _info(s, h_samp=hs, v_samp=vs, components=1 if smp == "L" else 3, height=c[1], width=c[2]),
                content=content, sampling=smp)
    for gs in ((2, 2), (2, 1), (1, 2), (4, 4)):
        add(f"greyscale declaring {gs[0]}x{gs[1]}", "one component: one block per MCU whatever SOF says", lambda s: _info(s, components=1, h_samp=1, v_samp=1, blocks=35, blocks_per_mcu=1),
            content=("real", 40, 56, 0), sampling="L", grey_sampling=gs)
    # restart intervals
    add("restart interval 1", "35 segments: RST7 wraps to RST0 four times", lambda s: _info(s, segments=35), restart=1)
    add("one MCU row per segment", "interval 7", lambda s: _info(s, segments=5, mcus_x=7), restart=7)
    add("restart interval 1, 4:2:0, unary tables", "12 segments of six blocks", lambda s: _info(s, segments=12, blocks_per_mcu=6) and s.st["max_ac_code"] == 16,
        sampling="420", restart=1, tables={k: "unary" for k in ((0, 0), (0, 1), (1, 0), (1, 1))})
    add("greyscale, restart interval 2", "18 segments, RST7 wraps twice", lambda s: _info(s, segments=18, components=1), sampling="L", restart=2)
    # the schedule's bound
    side = never_synchronising_side()
    add("never synchronising, one segment", "reversed tables shared by all components: as many rounds as subsequences, more than the workgroup has threads",
        lambda s: s.st["subsequences"] > D.THREADS and s.st["rounds"] == s.st["subsequences"] and s.st["max_ac_code"] == 16, f=never_synchronising(side))
    add("never synchronising, restart interval 2", "the same stream in many segments of a few rounds each",
        lambda s: _info(s, segments=-(-s.meta["mcus"] // 2)) and min(s.st["segment_rounds"]) >= 3 and max(s.st["segment_subsequences"]) <= 8,
        f=never_synchronising(side, restart=2))
    # segment lengths on the subsequence grid
    for res, (seed, k) in sorted(grid_seeds().items()):
        add(f"segment length {res} mod 128", f"segment {k} ends {({0: 'on', 1: 'one byte behind', 127: 'one byte in front of'})[res]} a subsequence boundary",
            lambda s, res=res, k=k: s.st["segment_bytes"][k] % S_BYTES == res and s.st["segment_subsequences"][k] >= 2 and s.st["segment_bytes"] == s.meta["segment_bytes"],
            content=GRID_CONTENT + (seed,), restart=GRID_RESTART)

    def extreme(s):
        sym = np.array(s.symbols)
        inner = sym[sym[:, 1] <= (s.st["subsequences"] - 1) * D.S]
        return len(inner) and (inner[:, 0] % D.S == D.S - 1).any() and (inner[:, 1] % D.S == 0).any()
    add("extreme symbol positions", "a symbol begins on the last bit of a subsequence, another ends on a boundary", extreme, content=("noise", 33, 15, extreme_seed()))
    # padding
    for pad in ("zeros", "random"):
        for smp in ("444", "420"):
            for ri in (0, 2):
                add(f"{pad} padding, {smp}, restart {ri}", "padding bits that are not all 1", lambda s, ri=ri: _info(s, restart_interval=ri) and s.padding_not_ones >= 1,
                    sampling=smp, pad=pad, restart=ri, seed=14)
    add("zero padding, unary tables, 33x15", "0 is the one-bit code of both classes: the padding is symbols", lambda s: s.padding_not_ones == 1 and all(s.P["huff"][k][0][0] == 1 for k in range(4)),
        content=("noise", 33, 15, 0), pad="zeros", tables={k: "unary" for k in ((0, 0), (0, 1), (1, 0), (1, 1))})
    add("flat greyscale, padding like a block", "three blocks of 6 bits, then 001010: DC 0 and EOB once more", lambda s: _info(s, blocks=3) and s.st["segment_bytes"] == [3] and s.st["blocks_past_the_last"] == 1,
        content=("flat", 7, 17, 0), sampling="L", pad="001010")
    add("flat greyscale, zero padding, restart 1", "blocks of 6 bits and 2 zero bits behind each", lambda s: _info(s, segments=6) and s.st["segment_bytes"] == [1] * 6 and s.padding_not_ones == 6,
        content=("flat", 16, 17, 0), sampling="L", pad="zeros", restart=1)
    # what stays refused
    add("spare 00 00 before EOI", "two whole bytes behind the padding", lambda s: s.st["segment_bytes"][-1] == s.meta["segment_bytes"][-1] and s.data[s.P["scan"][1] - 2:s.P["scan"][1]] == b"\x00\x00", spare=b"\x00\x00")
    add("spare FF before EOI", "FF 00 behind the padding", lambda s: s.data[s.P["scan"][1] - 2:s.P["scan"][1]] == b"\xff\x00" and s.P["segments"][0][-1] == 0xff, spare=b"\xff")
    add("spare 00 before every RSTn, 4:2:0", "a whole byte behind the padding of every segment", lambda s: _info(s, segments=6) and all(x[-1] == 0 for x in s.P["segments"]),
        sampling="420", restart=2, spare=b"\x00", spare_where="all")
    add("zero padding and a spare 00", "both at once", lambda s: s.P["segments"][0][-1] == 0, pad="zeros", spare=b"\x00")
    add("flat greyscale, whole spare blocks", "three blocks of 6 bits, 001010 and a spare 00101000: two more blocks, 14 bits left at the first",
        lambda s: _info(s, blocks=3) and s.st["segment_bytes"] == [4] and s.st["blocks_past_the_last"] == 2, content=("flat", 7, 17, 0), sampling="L", pad="001010", spare=b"\x28")
    add("no EOI", "the file ends behind the padding", lambda s: s.P is None and b"\xff\xd9" not in s.data[-8:], eoi=False)
    add("no EOI, zero padding, restart markers", "the same with RSTn in the scan", lambda s: s.P is None and b"\xff\xd9" not in s.data[-8:], eoi=False, pad="zeros", restart=7)
    return tuple(out)


def seen(entry):
    return _seen(entry.name)


@functools.lru_cache(maxsize=None)
def _seen(name):
    """What the checks look at: the parser's dict (None where it refuses), the schedule's status and statistics, the symbols of
    the writing pass, and how many segments have padding bits that are not all 1 (from the writer's own bit counts)."""
    entry = next(e for e in catalogue() if e.name == name)
    try:
        P = D.parse(entry.data)
    except D.Refused:
        return Seen(entry.data, entry.meta, None, None, None, None, 0)
    dec = D.Decoder(P)
    dec.symbols = []
    _, status, st = dec.fixed_point()
    odd = 0
    for seg, pos in zip(P["segments"], entry.meta["symbol_bits"]):
        n = int(pos[-1])
        tail = np.unpackbits(np.frombuffer(seg, np.uint8))[n:-(-n // 8) * 8]
        odd += bool(len(tail) and not tail.all())
    return Seen(entry.data, entry.meta, P, st, status, dec.symbols, odd)


def refusal(entry):
    """None for a file that must decode, else (class, code)."""
    return MUST_REFUSE.get(entry.name)
