"""numpy / Python statement of the baseline JPEG decoder (csrc/jpeg_decode.hip.h), stage by stage: the marker walk with its refusal
codes, the packed stream the kernels read, the Huffman state step, a plain serial decode, the subsequence schedule with its fixed
point, the DC sums, dequantisation and jidctint (idct_islow below), libjpeg's upsampling
and colour conversion.  tests/test_jpeg_decode_cpu.py holds it to Pillow and the library's host functions to it;
tests/test_jpeg_decode_gpu.py holds the kernels to it and to Pillow."""
import functools
import io
import struct

import numpy as np

from jpeg_encode_model import ZIGZAG, make_content  # noqa: F401  (make_content: the contents the tests decode)

S = 1024                                # JPEG_DEC_SUBSEQ_BITS
THREADS = 256                           # JPEG_DEC_THREADS
OFF_QUANT, OFF_SEL, OFF_HUFF, HUFF_BYTES = 64, 320, 336, 912
OFF_SEG = OFF_HUFF + 4 * HUFF_BYTES
INFO_FIELDS = ("width", "height", "components", "h_samp", "v_samp", "restart_interval", "blocks_per_mcu", "blocks", "segments",
               "packed_bytes", "entropy_bytes", "mcus_x", "mcus_y", "subsequences", "subsequence_bits", "reserved")
UNSUP_SOF, UNSUP_ARITHMETIC, UNSUP_PRECISION, UNSUP_COLOUR, UNSUP_SAMPLING, UNSUP_SCANS, UNSUP_QUANT16, UNSUP_SIZE = range(1, 9)
BAD_SOI, BAD_SEGMENT, BAD_TABLE, BAD_NO_SOS, BAD_NO_EOI, BAD_HEADER, BAD_RESTART = range(-1, -8, -1)
ST_CATEGORY, ST_NO_CODE, ST_WRITE, ST_BLOCK_TOTAL, ST_ROUNDS = 1, 2, 4, 8, 16


def idct_islow(coef, qt):
    """jidctint.c jpeg_idct_islow on (..., 8, 8) quantised coefficients: dequantise, pass 1 over columns, pass 2 over rows -> the
    samples before + 128 and the range limit (libjpeg-turbo's SIMD limit is a plain clamp of x + 128 to 0..255)."""
    CONST_BITS, PASS1_BITS = 13, 2
    F0298, F0390, F0541, F0765, F0899, F1175 = 2446, 3196, 4433, 6270, 7373, 9633
    F1501, F1847, F1961, F2053, F2562, F3072 = 12299, 15137, 16069, 16819, 20995, 25172

    def one(v, n):
        z1 = (v[..., 2] + v[..., 6]) * F0541
        t2, t3 = z1 - v[..., 6] * F1847, z1 + v[..., 2] * F0765
        t0, t1 = (v[..., 0] + v[..., 4]) << CONST_BITS, (v[..., 0] - v[..., 4]) << CONST_BITS
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
        z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
        z5 = (z3 + z4) * F1175
        a0, a1, a2, a3 = a0 * F0298, a1 * F2053, a2 * F3072, a3 * F1501
        z1, z2, z3, z4 = z1 * -F0899, z2 * -F2562, z3 * -F1961 + z5, z4 * -F0390 + z5
        a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
        o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
        return np.stack([(x + (1 << (n - 1))) >> n for x in o], -1)
    d = coef.astype(np.int64) * qt
    ws = one(d.swapaxes(-1, -2), CONST_BITS - PASS1_BITS).swapaxes(-1, -2)
    return one(ws, CONST_BITS + PASS1_BITS + 3)


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def build_table(bits, vals):
    """jdhuff.c jpeg_make_d_derived_tbl -> (look[256] uint16, maxcode[18], valoff[18], vals[256]) or None when the counts describe no
    prefix code."""
    look, v = np.zeros(256, np.uint16), np.zeros(256, np.uint8)
    maxcode, valoff = np.zeros(18, np.int32), np.zeros(18, np.int32)
    if sum(bits) > 256 or sum(bits) != len(vals):
        return None
    v[:len(vals)] = list(vals)
    code = k = 0
    maxcode[0] = -1
    for length in range(1, 17):
        n = bits[length - 1]
        if code + n > (1 << length):
            return None
        valoff[length] = k - code
        for _ in range(n):
            if length <= 8:
                look[code << (8 - length):(code + 1) << (8 - length)] = (length << 8) | vals[k]
            k += 1
            code += 1
        maxcode[length] = code - 1 if n else -1
        code <<= 1
    maxcode[17] = 0x7fffffff
    return look, maxcode, valoff, v


def parse(data):
    """The marker walk of jpeg_dec::parse: a dict (info words by name, tables, the scan's byte range) or Refused(code)."""
    f, n = data, len(data)
    if n < 4 or f[0] != 0xff or f[1] != 0xd8:
        raise Refused(BAD_SOI)
    pos, jfif, adobe, adobe_transform, sof, restart = 2, False, False, 0, None, 0
    quant, huff = {}, {}
    while True:
        if pos + 2 > n:
            raise Refused(BAD_NO_SOS)
        if f[pos] != 0xff:
            raise Refused(BAD_SEGMENT)
        m = f[pos + 1]
        if m == 0xff:
            pos += 1
            continue
        pos += 2
        if m == 0xd9:
            raise Refused(BAD_NO_SOS)
        if m in (0xd8, 0x01) or 0xd0 <= m <= 0xd7:
            continue
        if pos + 2 > n:
            raise Refused(BAD_SEGMENT)
        L = (f[pos] << 8) | f[pos + 1]
        if L < 2 or pos + L > n:
            raise Refused(BAD_SEGMENT)
        d = f[pos + 2:pos + L]
        if m == 0xc0:
            if sof is not None or len(d) < 6:
                raise Refused(BAD_HEADER)
            if d[0] != 8:
                raise Refused(UNSUP_PRECISION)
            height, width, nc = (d[1] << 8) | d[2], (d[3] << 8) | d[4], d[5]
            if width == 0 or height == 0 or nc == 0 or len(d) != 6 + 3 * nc:
                raise Refused(BAD_HEADER)
            if nc not in (1, 3):
                raise Refused(UNSUP_COLOUR)
            comps = [(d[6 + 3 * c], d[7 + 3 * c] >> 4, d[7 + 3 * c] & 15, d[8 + 3 * c]) for c in range(nc)]
            if any(not (1 <= h <= 4 and 1 <= v <= 4 and tq <= 3) for _, h, v, tq in comps):
                raise Refused(BAD_HEADER)
            sof = (width, height, comps)
        elif m == 0xc4:
            o = 0
            while o < len(d):
                if o + 17 > len(d):
                    raise Refused(BAD_SEGMENT)
                tc, th = d[o] >> 4, d[o] & 15
                if tc > 1 or th > 3:
                    raise Refused(BAD_HEADER)
                if th > 1:
                    raise Refused(UNSUP_SOF)
                cnt = sum(d[o + 1:o + 17])
                if cnt > 256 or o + 17 + cnt > len(d):
                    raise Refused(BAD_SEGMENT)
                huff[2 * tc + th] = (list(d[o + 1:o + 17]), list(d[o + 17:o + 17 + cnt]))
                o += 17 + cnt
        elif 0xc9 <= m <= 0xcf:
            raise Refused(UNSUP_ARITHMETIC)
        elif 0xc1 <= m <= 0xc8:
            raise Refused(UNSUP_PRECISION if m == 0xc1 and len(d) >= 1 and d[0] == 12 else UNSUP_SOF)
        elif m == 0xdb:
            o = 0
            while o < len(d):
                pq, tq = d[o] >> 4, d[o] & 15
                if pq > 1 or tq > 3:
                    raise Refused(BAD_HEADER)
                if pq == 1:
                    raise Refused(UNSUP_QUANT16)
                if o + 65 > len(d):
                    raise Refused(BAD_SEGMENT)
                q = np.zeros(64, np.uint8)
                q[ZIGZAG] = list(d[o + 1:o + 65])
                quant[tq] = q
                o += 65
        elif m == 0xdd:
            if len(d) != 2:
                raise Refused(BAD_SEGMENT)
            restart = (d[0] << 8) | d[1]
        elif m == 0xe0:
            if len(d) >= 14 and bytes(d[:5]) == b"JFIF\0":
                jfif = True
        elif m == 0xee:
            if len(d) >= 12 and bytes(d[:5]) == b"Adobe":
                adobe, adobe_transform = True, d[11]
        elif m == 0xda:
            if sof is None:
                raise Refused(BAD_HEADER)
            if len(d) < 1:
                raise Refused(BAD_SEGMENT)
            ns = d[0]
            width, height, comps = sof
            if ns < 1 or ns > 4 or len(d) != 1 + 2 * ns + 3:
                raise Refused(BAD_SEGMENT)
            if ns != len(comps):
                raise Refused(UNSUP_SCANS)
            sel = np.zeros(16, np.uint8)
            for c, (cid, _, _, tq) in enumerate(comps):
                if d[1 + 2 * c] != cid:
                    raise Refused(BAD_HEADER)
                td, ta = d[2 + 2 * c] >> 4, d[2 + 2 * c] & 15
                if td > 1 or ta > 1:
                    raise Refused(BAD_HEADER if td > 3 or ta > 3 else UNSUP_SOF)
                if td not in huff or 2 + ta not in huff or tq not in quant:
                    raise Refused(BAD_TABLE)
                if build_table(*huff[td]) is None or build_table(*huff[2 + ta]) is None:
                    raise Refused(BAD_HEADER)
                sel[4 * c:4 * c + 3] = (tq, td, 2 + ta)
            if tuple(d[1 + 2 * ns:]) != (0, 63, 0):
                raise Refused(BAD_HEADER)
            pos += L
            break
        pos += L
    width, height, comps = sof
    hs = vs = 1
    if len(comps) == 3:
        # libjpeg's rule (jdapimin.c): JFIF says YCbCr; else Adobe's transform byte; else the component ids
        ids = tuple(c[0] for c in comps)
        rgb = False if jfif else (adobe_transform == 0 if adobe else ids == (ord("R"), ord("G"), ord("B")))
        if rgb:
            raise Refused(UNSUP_COLOUR)
        hs, vs = comps[0][1], comps[0][2]
        if any((c[1], c[2]) != (1, 1) for c in comps[1:]) or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
            raise Refused(UNSUP_SAMPLING)
    # the entropy-coded bytes, unstuffed, cut at the RSTn markers
    segs, cur, q, nxt = [], bytearray(), pos, -1
    while q < n:
        if f[q] != 0xff:
            cur.append(f[q])
            q += 1
            continue
        if q + 1 >= n:
            break
        b = f[q + 1]
        if b == 0:
            cur.append(0xff)
            q += 2
        elif b == 0xff:
            q += 1
        elif 0xd0 <= b <= 0xd7:
            segs.append(bytes(cur))
            cur = bytearray()
            q += 2
        else:
            nxt = b
            break
    if nxt < 0:
        raise Refused(BAD_NO_EOI)
    segs.append(bytes(cur))
    if nxt != 0xd9:
        raise Refused(UNSUP_SCANS)
    ent = sum(len(s) for s in segs)
    if ent > 1 << 28:
        raise Refused(UNSUP_SIZE)
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    bpm = 1 if len(comps) == 1 else hs * vs + 2
    nmcu = mx * my
    nseg = -(-nmcu // restart) if restart else 1
    if len(segs) != nseg:
        raise Refused(BAD_RESTART)
    nsub = sum(-(-len(s) * 8 // S) for s in segs)
    info = dict(zip(INFO_FIELDS, (width, height, len(comps), hs, vs, restart, bpm, nmcu * bpm, nseg,
                                  OFF_SEG + 16 * nseg + -(-ent // 4) * 4, ent, mx, my, nsub, S, 0)))
    return dict(info=info, quant=quant, huff=huff, sel=sel, segments=segs, scan=(pos, q))


def pack(data):
    """The bytes jpeg_dec::pack writes."""
    P = parse(data)
    i = P["info"]
    out = bytearray(struct.pack("<16i", *(i[k] for k in INFO_FIELDS)))
    for t in range(4):
        out += bytes(P["quant"].get(t, np.zeros(64, np.uint8)))
    out += bytes(P["sel"])
    for s in range(4):
        if s in P["huff"]:
            look, maxcode, valoff, v = build_table(*P["huff"][s])
            out += look.astype("<u2").tobytes() + maxcode.astype("<i4").tobytes() + valoff.astype("<i4").tobytes() + v.tobytes()
        else:
            out += bytes(HUFF_BYTES)
    off = sub = 0
    nmcu, ri = i["mcus_x"] * i["mcus_y"], i["restart_interval"]
    for k, s in enumerate(P["segments"]):
        out += struct.pack("<4I", off * 8, len(s) * 8, sub, min(ri, nmcu - k * ri) if ri else nmcu)
        off += len(s)
        sub += -(-len(s) * 8 // S)
    ent = b"".join(P["segments"])
    out += ent + b"\xff" * (-len(ent) % 4)
    assert len(out) == i["packed_bytes"]
    return bytes(out)


class Decoder:
    """The state step f of csrc/jpeg_decode.hip.h over one file.  A state is (p, b, z): bit position in the unstuffed stream, block
    inside the MCU, zigzag position (0: a DC code is next)."""

    def __init__(self, P):
        self.P, i = P, P["info"]
        ent = b"".join(P["segments"])
        bits = np.unpackbits(np.frombuffer(ent + b"\xff" * (-len(ent) % 4 + 8), np.uint8))
        # win[p]: the 32 bits from bit p on (1-bits past the end), for every p a decode can reach
        nb = len(ent) * 8 + 32
        w = np.zeros(nb, np.int64)
        for k in range(32):
            w = (w << 1) | bits[k:k + nb]
        self.win = w.tolist()
        self.bpm = i["blocks_per_mcu"]
        nluma = 1 if i["components"] == 1 else i["h_samp"] * i["v_samp"]
        self.comp = [0 if b < nluma else b - nluma + 1 for b in range(self.bpm)]
        # per table: the symbol and length of the code at the top of every 16-bit value, by the kernel's search (lookahead for
        # up to 8 bits, then maxcode / valoff); length 16 and symbol 0 with found = 0 where nothing matches
        self.lut = {}
        for s, (hb, hv) in P["huff"].items():
            look, maxcode, valoff, vals = build_table(hb, hv)
            v16 = np.arange(65536, dtype=np.int64)
            length = np.zeros(65536, np.int64)
            sym = np.zeros(65536, np.int64)
            e = look[v16 >> 8].astype(np.int64)
            length[e > 0], sym[e > 0] = e[e > 0] >> 8, e[e > 0] & 255
            for ln in range(9, 17):
                c = v16 >> (16 - ln)
                hit = (length == 0) & (c <= maxcode[ln])
                length[hit] = ln
                sym[hit] = vals[(c[hit] + valoff[ln]) & 255]
            found = length > 0
            length[~found] = 16
            self.lut[s] = ((found.astype(np.int64) << 16) | (length << 8) | sym).tolist()
        self.tabs = [(self.lut[int(P["sel"][4 * c + 1])], self.lut[int(P["sel"][4 * c + 2])]) for c in self.comp]
        self.max_code = [0, 0]                  # the longest DC and AC code a writing pass has met
        self.symbols = None                     # a list: gains (first bit, last bit + 1) of every symbol of a writing pass

    def step(self, p, b, z, end, seg_end, write=None):
        """f: whole symbols from (p, b, z) until p >= end -> (p, b, z, blocks completed).  ``write``: (coef rows of the segment,
        first block, status list, list that gains the bit position behind every completed block) - the pass on true states, which
        stores every coefficient and reports damage."""
        win, tabs, bpm, done = self.win, self.tabs, self.bpm, 0
        if write is not None:
            coef, blk0, status, ends = write
            nblk = len(coef)
        while p < end:
            top = win[p]
            left = seg_end - p
            if left < 8 and (top >> (32 - left)) == (1 << left) - 1:
                p = seg_end
                break
            if write is not None and z == 0 and left < 8 and blk0 + done == nblk:
                p = seg_end                             # padding that is not 1-bits, behind the segment's last block
                break
            e = tabs[b][1 if z else 0][top >> 16]
            ln, sym = (e >> 8) & 255, e & 255
            size = sym & 15
            v = (top >> (32 - ln - size)) & ((1 << size) - 1)
            value = v - (1 << size) + 1 if size and v < (1 << (size - 1)) else v
            p += ln + size
            last = False
            if write is not None:
                k = 1 if z else 0
                self.max_code[k] = max(self.max_code[k], ln)
                if self.symbols is not None:
                    self.symbols.append((p - ln - size, p))
                if not e >> 16:
                    status[0] |= ST_NO_CODE
            if z == 0:
                if write is not None:
                    if sym > 11:
                        status[0] |= ST_CATEGORY
                    if blk0 + done < nblk:
                        coef[blk0 + done][0] = value
                    else:
                        status[0] |= ST_WRITE
                z = 1
            elif size == 0:
                if sym >> 4 == 15:
                    z += 16
                else:
                    last = True
            else:
                z += sym >> 4
                if write is not None:
                    if size > 10:
                        status[0] |= ST_CATEGORY
                    if z <= 63 and blk0 + done < nblk:
                        coef[blk0 + done][ZIGZAG[z]] = value
                    else:
                        status[0] |= ST_WRITE
                z += 1
            if last or z >= 64:
                if write is not None and blk0 + done >= nblk:
                    status[0] |= ST_BLOCK_TOTAL         # a whole block more than the segment has
                done += 1
                if write is not None:
                    ends.append(p)
                z = 0
                b = b + 1 if b + 1 < bpm else 0
        return p, b, z, done

    def segments(self):
        """(first bit, last bit + 1, subsequences, blocks, first block) of every restart segment."""
        i = self.P["info"]
        nmcu, ri, off = i["mcus_x"] * i["mcus_y"], i["restart_interval"], 0
        for k, s in enumerate(self.P["segments"]):
            mcus = min(ri, nmcu - k * ri) if ri else nmcu
            yield off * 8, (off + len(s)) * 8, -(-len(s) * 8 // S), mcus * self.bpm, k * ri * self.bpm
            off += len(s)

    def dc_sums(self, coef, nblk):
        """DC differences -> values, per component inside one segment's rows."""
        last = {}
        for g in range(nblk):
            c = self.comp[g % self.bpm]
            last[c] = coef[g][0] = ((last.get(c, 0) + coef[g][0] + 32768) & 0xffff) - 32768

    def serial(self):
        """One decoder walking every segment from its start -> ((blocks, 64) coefficients in natural order, status)."""
        out, status = [], [0]
        for p0, seg_end, n, nblk, _ in self.segments():
            coef = [[0] * 64 for _ in range(nblk)]
            p, b, z, done = p0, 0, 0, 0
            for i in range(n):
                p, b, z, d = self.step(p, b, z, min(p0 + (i + 1) * S, seg_end), seg_end, (coef, done, status, []))
                done += d
            if done < nblk:
                status[0] |= ST_BLOCK_TOTAL
            self.dc_sums(coef, nblk)
            out += coef
        return np.array(out, np.int64).reshape(-1, 64), status[0]

    def fixed_point(self):
        """The subsequence schedule of jpeg_dec_huff_kernel -> (coefficients, status, stats).  stats: rounds (the most over the
        segments, the last round that changes nothing included), decodes (subsequence decodes of pass 1 and the rounds),
        subsequences (the most in one segment), max_blocks_in_subsequence, max_block_bits (the longest block), last_segment_mcus;
        per segment: segment_rounds, segment_subsequences, segment_bytes (unstuffed); max_dc_code and max_ac_code (the longest
        code of either class the writing pass met); blocks_past_the_last (blocks the passes counted out of padding bits)."""
        out, status = [], [0]
        st = dict(rounds=0, decodes=0, subsequences=0, max_blocks_in_subsequence=0, max_block_bits=0, total=0, last_segment_mcus=0,
                  segment_rounds=[], segment_subsequences=[], segment_bytes=[], blocks_past_the_last=0)
        self.max_code = [0, 0]
        for p0, seg_end, n, nblk, _ in self.segments():
            end = [min(p0 + (i + 1) * S, seg_end) for i in range(n)]
            A = [self.step(p0 + i * S, 0, 0, end[i], seg_end) + (1,) for i in range(n)]
            st["decodes"] += n
            r, anyc = 0, True
            while anyc and r < n:
                r += 1
                B = []
                for i in range(n):
                    e = A[i][:4] + (0,)
                    if i > 0 and A[i - 1][4]:
                        new = self.step(A[i - 1][0], A[i - 1][1], A[i - 1][2], end[i], seg_end)
                        st["decodes"] += 1
                        e = new + (1 if new[:3] != A[i][:3] else 0,)
                    B.append(e)
                anyc = any(e[4] for e in B)
                A = B
            if anyc:
                status[0] |= ST_ROUNDS
            coef = [[0] * 64 for _ in range(nblk)]
            first, ends = 0, [p0]
            for i in range(n):
                start = (p0, 0, 0) if i == 0 else A[i - 1][:3]
                self.step(*start, end[i], seg_end, (coef, first, status, ends))
                first += A[i][3]
            if first < nblk:
                status[0] |= ST_BLOCK_TOTAL
            self.dc_sums(coef, nblk)
            out += coef
            counts = [a[3] for a in A]
            st["rounds"] = max(st["rounds"], r)
            st["subsequences"] = max(st["subsequences"], n)
            st["total"] += n
            st["max_blocks_in_subsequence"] = max([st["max_blocks_in_subsequence"]] + counts)
            st["max_block_bits"] = max([st["max_block_bits"]] + [b - a for a, b in zip(ends, ends[1:])])
            st["last_segment_mcus"] = nblk // self.bpm
            st["segment_rounds"].append(r)
            st["segment_subsequences"].append(n)
            st["segment_bytes"].append((seg_end - p0) // 8)
            st["blocks_past_the_last"] += max(first - nblk, 0)
        st["max_dc_code"], st["max_ac_code"] = self.max_code
        return np.array(out, np.int64).reshape(-1, 64), status[0], st


def reconstruct(P, coef, stats=None):
    """Coefficients (blocks in scan order, natural order, DC summed) -> the (H, W, 3) uint8 image libjpeg makes of them.  ``stats``
    (a dict) gains max_abs_idct, the largest IDCT output before + 128 and the range limit (above 128: the limit was reached)."""
    max_abs = 0
    i = P["info"]
    W, H, nc, hs, vs, bpm, mx, my = (i[k] for k in ("width", "height", "components", "h_samp", "v_samp", "blocks_per_mcu", "mcus_x", "mcus_y"))
    nluma = 1 if nc == 1 else hs * vs
    c = coef.reshape(my, mx, bpm, 8, 8)
    planes = []
    for comp in range(nc):
        qt = P["quant"][int(P["sel"][4 * comp])].astype(np.int64).reshape(8, 8)
        if comp == 0:
            b = c[:, :, :nluma].reshape(my, mx, vs, hs, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my * vs, mx * hs, 8, 8)
        else:
            b = c[:, :, nluma + comp - 1]
        x = idct_islow(b, qt)
        max_abs = max(max_abs, int(np.abs(x).max()))
        px = np.clip(x + 128, 0, 255)
        planes.append(px.swapaxes(1, 2).reshape(b.shape[0] * 8, b.shape[1] * 8))
    if stats is not None:
        stats["max_abs_idct"] = max_abs
    Y = planes[0][:H, :W]
    if nc == 1:
        return np.ascontiguousarray(np.repeat(Y[..., None], 3, axis=2).astype(np.uint8))
    rw, rh = -(-W // hs), -(-H // vs)                      # the real downsampled size

    def up(p):
        p = p[:rh, :rw]
        if hs == 1:
            return p
        if rw <= 2:                                       # jdsample.c: plain replication for so narrow a component
            return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)[:H, :W]
        if vs == 1:                                       # h2v1_fancy_upsample
            left, right = np.hstack([p[:, :1], p[:, :-1]]), np.hstack([p[:, 1:], p[:, -1:]])
            o = np.empty((rh, 2 * rw), np.int64)
            o[:, 0::2], o[:, 1::2] = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
            return o[:H, :W]
        above, below = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
        cs = np.empty((2 * rh, rw), np.int64)
        cs[0::2], cs[1::2] = 3 * p + above, 3 * p + below
        left, right = np.hstack([cs[:, :1], cs[:, :-1]]), np.hstack([cs[:, 1:], cs[:, -1:]])
        o = np.empty((2 * rh, 2 * rw), np.int64)
        o[:, 0::2], o[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
        return o[:H, :W]

    xb, xr = up(planes[1]) - 128, up(planes[2]) - 128
    out = np.stack([Y + ((91881 * xr + 32768) >> 16), Y + ((-22554 * xb + 32768 - 46802 * xr) >> 16), Y + ((116130 * xb + 32768) >> 16)], -1)
    return np.ascontiguousarray(np.clip(out, 0, 255).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def decode_full(data):
    """(image, stats) of the bytes of a file by the subsequence schedule; raises Refused for a file the parser or the entropy data
    refuses (code: the status bits, negated by 1000 to tell them from the parser's)."""
    P = parse(data)
    coef, status, st = Decoder(P).fixed_point()
    if status:
        raise Refused(1000 + status)
    return reconstruct(P, coef, st), st


def decode(data, crop=None, bgr=False):
    img, _ = decode_full(bytes(data))
    if crop is not None:
        x0, y0, w, h = crop
        img = img[y0:y0 + h, x0:x0 + w]
    return np.ascontiguousarray(img[..., ::-1] if bgr else img)


def pillow_decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def pillow_file(kind, H, W, q, sub, seed=0, **kw):
    """The bytes Pillow saves for make_content(kind, H, W, seed): sub 0, 1, 2, or "L" for a greyscale file; kw: optimize,
    restart_marker_blocks, restart_marker_rows, progressive."""
    from PIL import Image
    img = make_content(kind, H, W, seed)
    buf = io.BytesIO()
    if sub == "L":
        Image.fromarray(img[..., 1]).save(buf, "JPEG", quality=q, **kw)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=sub, **kw)
    return buf.getvalue()


# ---- the test matrix: every value of every axis, not the full product --------------------------------------------------------------
SIZES = ((1, 1), (8, 8), (9, 7), (16, 16), (17, 17), (33, 15), (40, 56), (64, 64), (250, 131))
SUBSAMPLINGS = (0, 1, 2, "L")
QUALITIES = (1, 10, 50, 75, 95, 100)
CONTENTS = ("noise", "real", "gradient", "flat")
SETTINGS = ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1})


def matrix():
    """(kind, H, W, q, sub, settings) - every size with every subsampling, the other axes cycling with strides that are coprime to
    their lengths, so that each of their values meets each size and each subsampling over the list."""
    out, n = [], 0
    for H, W in SIZES:
        for sub in SUBSAMPLINGS:
            out.append((CONTENTS[n % 4], H, W, QUALITIES[(5 * n + n // 6) % 6], sub, SETTINGS[(n + n // 4) % 4]))
            n += 1
    return out


def bw_noise(H, W, seed=5):
    """Black and white pixel noise, the same in the three channels: at quality 100 its luma blocks take more than 1024 bits."""
    g = (np.random.RandomState(seed).randint(0, 2, (H, W)) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


def long_blocks_file(H=16, W=16, seed=3):
    """A 4:4:4 quality-100 file written by the encoder model from made-up coefficients: 44 luma coefficients of 256..399 per block
    cost 25 bits each (a 16-bit code and 9 magnitude bits), so every luma block is longer than one subsequence.  No image has such
    blocks behind Pillow's tables; libjpeg decodes them all the same, saturating."""
    import jpeg_encode_model as E
    rs = np.random.RandomState(seed)
    nb = (H // 8) * (W // 8)
    blocks = np.zeros((nb * 3, 64), np.int64)
    for g in range(0, nb * 3, 3):
        blocks[g, 0] = rs.randint(-200, 200)
        blocks[g, 1:45] = rs.randint(256, 400, 44) * rs.choice([-1, 1], 44)
    vals, lens, _ = E.entropy(blocks, np.tile([0, 1, 1], nb), 0)
    return E.header(H, W, 100, 0) + E.pack(vals, lens) + b"\xff\xd9"


def damaged(data, seed):
    """The damaged copies tools/jpeg_decode_host_check.cpp walks, byte for byte: one (seed 1..3) or eight (4..6) bit flips inside
    the entropy-coded bytes, placed by a linear congruential generator."""
    lo, hi = parse(data)["scan"]
    d, x = bytearray(data), (seed * 2654435761) & 0xffffffff
    for _ in range(1 if seed <= 3 else 8):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        at = lo + (x >> 8) % (hi - lo)
        x = (x * 1664525 + 1013904223) & 0xffffffff
        d[at] ^= 1 << ((x >> 13) & 7)
    return bytes(d)
