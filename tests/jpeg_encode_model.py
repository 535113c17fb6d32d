"""numpy statement of the baseline JPEG encoder (csrc/jpeg_encode.hip.h): libjpeg's path from an (H, W, 3) uint8 image to the bytes of
the file Pillow's Image.save(JPEG, quality=q, subsampling=0 or 2) writes - colour conversion, edge padding, jfdctint and quantisation
(the arithmetic of tests/test_jpeg_roundtrip_cpu.py, imported), the dummy blocks of jccoefct.c, Huffman symbols from the Annex K
tables (jchuff.c encode_one_block), bit packing, the 1-bit padding of flush_bits, byte stuffing and the header (jcmarker.c).
tests/test_jpeg_encode_cpu.py holds it to Pillow; tests/test_jpeg_encode_gpu.py holds the kernels to it and to Pillow."""
import io
import os

import numpy as np

from test_jpeg_roundtrip_cpu import STD_CHROMA, STD_LUMA, _blocks, fdct, quant_table, quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BLOCK_BITS = 22 + 63 * 26          # 11-bit DC code + 11 magnitude bits, 63 x (16-bit AC code + 10 magnitude bits)
HEADER_BYTES = 623

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

# Annex K.3: number of codes of each length 1..16, then the symbols in code order
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344454647"
    "48494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
    "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def huff_codes(bits, vals):
    """jchuff.c jpeg_make_c_derived_tbl: symbol -> (code, length), codes of one length consecutive, doubled at each longer length."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [huff_codes(DC_BITS[t], DC_VALS) for t in range(2)]
AC_CODES = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def header(H, W, q, sub):
    """SOI, APP0 (JFIF 1.01, no units, 1 x 1), DQT luma, DQT chroma, SOF0, DHT DC0 AC0 DC1 AC1, SOS."""
    o = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t, std in enumerate((STD_LUMA, STD_CHROMA)):
        o += bytes([0xff, 0xdb, 0, 67, t]) + bytes(quant_table(std, q).ravel()[ZIGZAG].tolist())
    o += bytes([0xff, 0xc0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22 if sub else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in range(2):
        o += bytes([0xff, 0xc4, 0, 31, t]) + bytes(DC_BITS[t]) + bytes(DC_VALS)
        o += bytes([0xff, 0xc4, 0, 181, 0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t])
    o += bytes([0xff, 0xda, 0, 12, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(o) == HEADER_BYTES
    return bytes(o)


def coefficients(img, q, sub, bgr=False):
    """The quantised coefficients libjpeg hands its entropy coder: (nblk, 64) int64 in zigzag order, blocks in scan order
    (4:4:4: Y Cb Cr per 8 x 8 MCU; 4:2:0: Y0 Y1 Y2 Y3 Cb Cr per 16 x 16 MCU), and the component (0 luma, 1 chroma) of each."""
    a = img.astype(np.int64)
    if bgr:
        a = a[..., ::-1]
    H, W = a.shape[:2]
    R, G, B = a[..., 0], a[..., 1], a[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    qts = [quant_table(STD_LUMA, q), quant_table(STD_CHROMA, q)]

    def coef(plane, t):                # (by, bx, 64) zigzag
        c = quantize(fdct(_blocks(plane) - 128), qts[t])
        return c.reshape(c.shape[0], c.shape[1], 64)[..., ZIGZAG]

    if sub == 0:
        # jcsample.c fullsize_downsample: a copy, right edge replicated to a multiple of 8; jcprepct.c replicates the last row
        H8, W8 = -(-H // 8) * 8, -(-W // 8) * 8
        cs = [coef(np.pad(p, ((0, H8 - H), (0, W8 - W)), mode="edge"), t) for p, t in ((Y, 0), (Cb, 1), (Cr, 1))]
        blocks = np.stack(cs, 2).reshape(-1, 64)
        comp = np.tile([0, 1, 1], blocks.shape[0] // 3)
        return blocks, comp
    H16, W16 = -(-H // 16) * 16, -(-W // 16) * 16

    def down(c):                       # jcprepct.c + jcsample.c h2v2_downsample, as in the round trip
        He = H + (H & 1)
        c = np.pad(c, ((0, He - H), (0, W16 - W)), mode="edge")
        bias = np.tile([1, 2], W16 // 4)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        return np.pad(d, ((0, H16 // 2 - He // 2), (0, 0)), mode="edge")

    cy = coef(np.pad(Y, ((0, H16 - H), (0, W16 - W)), mode="edge"), 0)
    cb, cr = coef(down(Cb), 1), coef(down(Cr), 1)
    # jccoefct.c compress_data: luma blocks beyond the component's real size in blocks are dummies - no AC, the DC of the block to
    # their left (right edge) or of the last block of the row above inside the MCU (bottom edge)
    bh, bw = -(-H // 8), -(-W // 8)
    my, mx = H16 // 16, W16 // 16
    out = np.zeros((my, mx, 6, 64), np.int64)
    for j in range(my):
        for i in range(mx):
            y = [cy[2 * j, 2 * i], cy[2 * j, 2 * i + 1], cy[2 * j + 1, 2 * i], cy[2 * j + 1, 2 * i + 1]]
            if 2 * i + 1 >= bw:
                y[1] = np.zeros(64, np.int64)
                y[1][0] = y[0][0]
            if 2 * j + 1 >= bh:
                for k in (2, 3):
                    y[k] = np.zeros(64, np.int64)
                    y[k][0] = y[1][0]
            elif 2 * i + 1 >= bw:
                y[3] = np.zeros(64, np.int64)
                y[3][0] = y[2][0]
            out[j, i, :4] = y
            out[j, i, 4], out[j, i, 5] = cb[j, i], cr[j, i]
    blocks = out.reshape(-1, 64)
    return blocks, np.tile([0, 0, 0, 0, 1, 1], my * mx)


def _nbits(v):
    return int(abs(int(v))).bit_length()


def entropy(blocks, comp, sub, stats=None):
    """encode_one_block over the scan: the (value, bit count) pairs in emission order and the bit count of every block.  ``stats``
    (a dict) collects which arms were reached."""
    st = stats if stats is not None else {}
    for k in ("eob_only", "zrl", "no_eob", "run15", "run16", "max_dc_cat", "max_ac_size", "blocks_3zrl_no_eob"):
        st.setdefault(k, 0)
    vals, lens, block_bits = [], [], []
    last_dc = {}
    for g in range(blocks.shape[0]):
        c = blocks[g]
        t = int(comp[g])
        ci = g % 3 if sub == 0 else max(g % 6 - 3, 0)      # the component: DC is predicted per component
        n0 = len(lens)

        def put(code_len, v, s):
            code, length = code_len
            mag = (int(v) - 1 if v < 0 else int(v)) & ((1 << s) - 1)
            vals.append((code << s) | mag)
            lens.append(length + s)

        diff = int(c[0]) - last_dc.get(ci, 0)
        last_dc[ci] = int(c[0])
        assert abs(diff) <= 2047, diff                   # category 11 is the last one of the baseline DC tables
        s = _nbits(diff)
        st["max_dc_cat"] = max(st["max_dc_cat"], s)
        put(DC_CODES[t][s], diff, s)
        zrl = prev = 0
        nz = np.flatnonzero(c[1:]) + 1
        for k in nz:
            v = int(c[k])
            assert abs(v) <= 1023, v                     # size 10 is the last one of the baseline AC tables
            r = int(k) - prev - 1                        # zeros since the last non-zero coefficient
            prev = int(k)
            if r == 16:
                st["run16"] += 1
            while r > 15:
                put(AC_CODES[t][0xf0], 0, 0)
                zrl += 1
                r -= 16
            if r == 15:
                st["run15"] += 1
            s = _nbits(v)
            st["max_ac_size"] = max(st["max_ac_size"], s)
            put(AC_CODES[t][(r << 4) | s], v, s)
        if len(nz) == 0 or nz[-1] != 63:
            put(AC_CODES[t][0], 0, 0)
            if len(nz) == 0:
                st["eob_only"] += 1
        else:
            st["no_eob"] += 1
            if zrl == 3 and len(nz) == 1:
                st["blocks_3zrl_no_eob"] += 1
        st["zrl"] += zrl
        block_bits.append(sum(lens[n0:]))
    return np.array(vals, np.int64), np.array(lens, np.int64), np.array(block_bits, np.int64)


def pack(vals, lens, stats=None):
    """The scan's bytes: codes packed most significant bit first, the last partial byte filled with 1-bits (flush_bits), then a
    0x00 after every 0xFF byte, the padded one included."""
    st = stats if stats is not None else {}
    pos = np.concatenate([[0], np.cumsum(lens)])
    nbits = int(pos[-1])
    bits = np.ones(-(-nbits // 8) * 8, np.uint8)
    bits[:nbits] = 0
    for t in range(int(lens.max())):
        m = lens > t
        bits[pos[:-1][m] + t] = (vals[m] >> (lens[m] - 1 - t)) & 1
    raw = np.packbits(bits)
    ff = np.flatnonzero(raw == 0xff)
    st["stuffed"] = len(ff)
    st["pad_bits"] = len(bits) - nbits
    st["pad_made_ff"] = bool(nbits % 8 and raw[-1] == 0xff)
    st["scan_bits"] = nbits
    return np.insert(raw, ff + 1, 0).tobytes()


def encode(img, q, sub, bgr=False, stats=None):
    """The whole file."""
    blocks, comp = coefficients(img, q, sub, bgr)
    vals, lens, block_bits = entropy(blocks, comp, sub, stats)
    assert block_bits.max() <= MAX_BLOCK_BITS
    H, W = img.shape[:2]
    return header(H, W, q, sub) + pack(vals, lens, stats) + b"\xff\xd9"


def bound(H, W, sub):
    """ucdir_jpeg_encode_bound: every block at its 1660 bits, every byte of the scan stuffed, header and EOI."""
    nblk = -(-H // 16) * -(-W // 16) * 6 if sub else -(-H // 8) * -(-W // 8) * 3
    return HEADER_BYTES + 2 * -(-nblk * MAX_BLOCK_BITS // 8) + 2


def pillow(img, q, sub, bgr=False):
    from PIL import Image
    a = np.ascontiguousarray(img[..., ::-1]) if bgr else img
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=q, subsampling=sub)
    return buf.getvalue()


# ---- contents, each there to reach one arm of the entropy coder -----------------------------------------------------------------
def basis_block(terms):
    """An 8 x 8 grey block 128 + sum of amp x the DCT basis function at zigzag position z, for (z, amp) in terms."""
    x = np.arange(8)
    f = np.zeros((8, 8))
    for z, amp in terms:
        v, u = divmod(int(ZIGZAG[z]), 8)
        f += amp * np.outer(np.cos((2 * x + 1) * v * np.pi / 16), np.cos((2 * x + 1) * u * np.pi / 16))
    return np.clip(np.round(128 + f), 0, 255).astype(np.uint8)


def grey_tiles(block, H, W):
    t = np.tile(block, (-(-H // 8), -(-W // 8)))[:H, :W]
    return np.ascontiguousarray(np.repeat(t[..., None], 3, axis=2))


def make_content(kind, H, W, seed=0):
    rs = np.random.RandomState(seed + 1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "flat":
        return np.full((H, W, 3), 128, np.uint8)
    if kind == "noise":
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "checker":              # 1-pixel black / white checkerboard
        return np.ascontiguousarray(np.repeat((((x + y) & 1) * 255)[..., None], 3, axis=2).astype(np.uint8))
    if kind == "bwblocks":             # 8 x 8 black and white squares: DC differences of category 11 at q = 100
        return np.ascontiguousarray(np.repeat(((((x >> 3) + (y >> 3)) & 1) * 255)[..., None], 3, axis=2).astype(np.uint8))
    if kind == "coef63":               # the only non-zero AC is the last one: ZRL ZRL ZRL, (14, s), no EOB
        return grey_tiles(basis_block([(63, 100)]), H, W)
    if kind == "run15":                # zigzag 1 and 17 non-zero: a run of exactly 15 zeros, no ZRL
        return grey_tiles(basis_block([(1, 40), (17, 40)]), H, W)
    if kind == "run16":                # zigzag 1 and 18 non-zero: a run of exactly 16 zeros, ZRL then run 0
        return grey_tiles(basis_block([(1, 40), (18, 40)]), H, W)
    if kind == "gradient":
        return np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(H + W - 2, 1)], -1).astype(np.uint8)
    if kind == "real":
        real = np.load(os.path.join(ROOT, "tests", "golden", "sid_real_image.npz"))["cond_u8"]
        reps = (-(-H // real.shape[0]), -(-W // real.shape[1]), 1)
        return np.ascontiguousarray(np.tile(real, reps)[:H, :W])
    if kind == "smooth":               # restored-image-like: a smooth image plus small noise
        base = 128 + 90 * np.sin(x / 37.0)[..., None] * np.cos(y / 29.0)[..., None] * np.array([1.0, 0.8, 0.6])
        return np.clip(base + rs.normal(0, 3, (H, W, 3)), 0, 255).astype(np.uint8)
    raise ValueError(kind)
