"""A plain-Python decoder of Zstandard payloads: the rules csrc/events_aedat4_zstd.hip states at its top (RFC 8878, no dictionary),
restated.  decode(payload, verify) -> (bytes, status) with the status words of the kernels: a damaged stream is CORRUPT, a wrong
content checksum CHECKSUM, and what was decoded before either is not returned.  Shares nothing with the kernels or with
tests/zstd_stream_writer.py but the format (the writer's XXH64 is cross-checked against the one below by the tests).
"""
import struct

CORRUPT, CHECKSUM = 1, 2
MAX_DECODED = (1 << 23) - 16
BLOCK_MAX = 1 << 17
M64 = (1 << 64) - 1

LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# (accuracy limit, symbols, predefined distribution, its accuracy)
LL, OF, ML = (9, 36, LL_NORM, 6), (8, 32, OF_NORM, 5), (9, 53, ML_NORM, 6)


class Corrupt(Exception):
    pass


def need(ok):
    if not ok:
        raise Corrupt()


# ------------------------------------------------------------------ XXH64
P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & M64


def _round(acc, v):
    return (_rotl((acc + v * P2) & M64, 31) * P1) & M64


def xxh64(data, seed=0):
    data = bytes(data)
    n, i = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed, (seed - P1) & M64]
        while i + 32 <= n:
            for k, w in enumerate(struct.unpack_from("<4Q", data, i)):
                v[k] = _round(v[k], w)
            i += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for k in range(4):
            h = ((h ^ _round(0, v[k])) * P1 + P4) & M64
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, i)[0]), 27) * P1 + P4) & M64
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, i)[0] * P1) & M64, 23) * P2 + P3) & M64
        i += 4
    while i < n:
        h = (_rotl(h ^ (data[i] * P5) & M64, 11) * P1) & M64
        i += 1
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    h ^= h >> 32
    return h


# ------------------------------------------------------------------ bitstreams
class Backward:
    """A backward bitstream: the highest set bit of the last byte is the end marker; bits are read from below it downwards and
    read as zeros below the first byte, which makes `left` negative."""

    def __init__(self, data):
        need(len(data) >= 1 and data[-1] != 0)
        self.value = int.from_bytes(data, "little")
        self.left = self.value.bit_length() - 1

    def peek(self, nb):
        lo = self.left - nb
        v = self.value >> lo if lo >= 0 else self.value << -lo
        return v & ((1 << nb) - 1)

    def read(self, nb):
        v = self.peek(nb)
        self.left -= nb
        return v


def fse_read_norm(data, max_log, max_syms):
    """An FSE table description at the start of data -> (probabilities, accuracy, bytes taken)."""
    value, total = int.from_bytes(data, "little"), 8 * len(data)
    bit = 0

    def take(nb):
        nonlocal bit
        v = (value >> bit) & ((1 << nb) - 1)
        bit += nb
        return v

    al = take(4) + 5
    need(al <= max_log)
    remaining, norm = 1 << al, []
    while remaining > 0 and len(norm) < max_syms:
        bits = (remaining + 1).bit_length()
        val = take(bits)
        lower, thresh = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        if (val & lower) < thresh:
            bit -= 1
            val &= lower
        elif val > lower:
            val -= thresh
        proba = val - 1
        remaining -= abs(proba)
        norm.append(proba)
        if proba == 0:
            while True:
                rep = take(2)
                norm += [0] * min(rep, max_syms - len(norm))
                if rep != 3 or len(norm) >= max_syms or bit > total:
                    break
        need(bit <= total)
    need(remaining == 0 and bit <= total)
    return norm, al, (bit + 7) >> 3


def fse_build(norm, log):
    """-> the decode table, a list of (symbol, bits, baseline)."""
    size = 1 << log
    need(sum(abs(c) for c in norm) == size)
    sym = [0] * size
    high = size - 1
    nxt = []
    for s, c in enumerate(norm):
        nxt.append(1 if c == -1 else c)
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    need(pos == 0)
    table = []
    for u in range(size):
        x = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb = log - (x.bit_length() - 1)
        table.append((sym[u], nb, (x << nb) - size))
    return table


def huffman_table(data):
    """A Huffman tree description at the start of data -> (table of (symbol, code length), maxbits, bytes taken)."""
    need(len(data) >= 1)
    h = data[0]
    if h >= 128:
        n = h - 127
        used = 1 + (n + 1) // 2
        need(used <= len(data))
        weights = [(data[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
    else:
        used = 1 + h
        need(h != 0 and used <= len(data))
        norm, al, head = fse_read_norm(data[1:used], 6, 256)
        t = fse_build(norm, al)
        b = Backward(data[1 + head:used])
        s1, s2 = b.read(al), b.read(al)
        need(b.left >= 0)
        weights = []
        while True:
            need(len(weights) < 254)
            weights.append(t[s1][0])
            if t[s1][1] > b.left:
                weights.append(t[s2][0])
                break
            s1 = t[s1][2] + b.read(t[s1][1])
            s1, s2 = s2, s1
    need(all(w <= 11 for w in weights))
    total = sum(1 << (w - 1) for w in weights if w)
    need(total > 0)
    maxbits = total.bit_length()
    need(maxbits <= 11)
    gap = (1 << maxbits) - total
    need(gap & (gap - 1) == 0)
    weights.append(gap.bit_length())
    table = []
    for w in range(1, maxbits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                table += [(s, maxbits + 1 - w)] * (1 << (w - 1))
    return table, maxbits, used


def huffman_stream(data, table, log, count):
    b = Backward(data)
    out = bytearray()
    for _ in range(count):
        need(b.left >= 0)
        s, nb = table[b.peek(log)]
        out.append(s)
        b.left -= nb
    need(b.left == 0)
    return bytes(out)


class Frame:
    def __init__(self, start, window):
        self.start, self.window = start, window
        self.rep = [1, 4, 8]
        self.huf = None                 # (table, log)
        self.seq = [None, None, None]   # (table, log) of LL, OF, ML
        self.have_seq = False


def compressed_block(f, b, out, limit, store):
    """One Compressed block b appended to out (a bytearray; a list of one length when store is false)."""
    bs = len(b)
    need(bs >= 1)
    ltype, fmt = b[0] & 3, (b[0] >> 2) & 3
    streams = 1
    if ltype < 2:
        hb = 2 if fmt == 1 else 3 if fmt == 3 else 1
        need(bs >= hb)
        regen = (b[0] >> 4) | (b[1] << 4) if fmt == 1 else (b[0] >> 4) | (b[1] << 4) | (b[2] << 12) if fmt == 3 else b[0] >> 3
        comp = regen if ltype == 0 else 1
    else:
        hb, nb = (3, 10) if fmt < 2 else (fmt + 2, 14 if fmt == 2 else 18)
        need(bs >= hb)
        v = int.from_bytes(b[:hb], "little")
        regen, comp = (v >> 4) & ((1 << nb) - 1), (v >> (4 + nb)) & ((1 << nb) - 1)
        streams = 1 if fmt == 0 else 4
    need(regen <= BLOCK_MAX and hb + comp <= bs)
    body = b[hb:hb + comp]
    lit = None
    if ltype == 0:
        lit = body
    elif ltype == 1:
        lit = bytes(body) * regen
    else:
        sp = 0
        if ltype == 2:
            if store:
                table, log, sp = huffman_table(body)
                f.huf = (table, log)
            else:
                f.huf = True
        else:
            need(f.huf is not None)
        if store:
            table, log = f.huf
            if streams == 1:
                lit = huffman_stream(body[sp:], table, log, regen)
            else:
                need(comp - sp >= 6)
                sizes = list(struct.unpack_from("<3H", body, sp))
                sizes.append(comp - sp - 6 - sum(sizes))
                each = (regen + 3) // 4
                counts = [each, each, each, regen - 3 * each]
                need(sizes[3] >= 1 and counts[3] >= 0)
                at, parts = sp + 6, []
                for size, count in zip(sizes, counts):
                    parts.append(huffman_stream(body[at:at + size], table, log, count))
                    at += size
                lit = b"".join(parts)
    sp = hb + comp
    need(sp < bs)
    nseq = b[sp]
    sp += 1
    if nseq >= 128:
        if nseq == 255:
            need(sp + 2 <= bs)
            nseq = b[sp] + (b[sp + 1] << 8) + 0x7F00
            sp += 2
        else:
            need(sp + 1 <= bs)
            nseq = ((nseq - 128) << 8) + b[sp]
            sp += 1
    start_len = len(out) if store else out[0]

    def size():
        return len(out) if store else out[0]

    used = 0

    def literals(count):
        nonlocal used
        if store:
            out.extend(lit[used:used + count])
        else:
            out[0] += count
        used += count

    if nseq == 0:
        need(sp == bs and size() + regen <= limit)
        literals(regen)
        return
    need(sp < bs)
    modes = b[sp]
    sp += 1
    need(modes & 3 == 0)
    for k, (kind, shift) in enumerate(((LL, 6), (OF, 4), (ML, 2))):
        mode = (modes >> shift) & 3
        max_log, max_syms, predef, predef_log = kind
        if mode == 0:
            f.seq[k] = (fse_build(predef, predef_log), predef_log)
        elif mode == 1:
            need(sp < bs and b[sp] < max_syms)
            f.seq[k] = ([(b[sp], 0, 0)], 0)
            sp += 1
        elif mode == 2:
            norm, al, n = fse_read_norm(b[sp:], max_log, max_syms)
            f.seq[k] = (fse_build(norm, al), al)
            sp += n
        else:
            need(f.have_seq)
    (tl, ll_log), (to, of_log), (tm, ml_log) = f.seq
    bits = Backward(b[sp:])
    sl, so, sm = bits.read(ll_log), bits.read(of_log), bits.read(ml_log)
    for i in range(nseq):
        cl, co, cm = tl[sl], to[so], tm[sm]
        ofv = (1 << co[0]) + bits.read(co[0])
        ml = ML_BASE[cm[0]] + bits.read(ML_BITS[cm[0]])
        ll = LL_BASE[cl[0]] + bits.read(LL_BITS[cl[0]])
        if i + 1 < nseq:
            sl = cl[2] + bits.read(cl[1])
            sm = cm[2] + bits.read(cm[1])
            so = co[2] + bits.read(co[1])
        need(bits.left >= 0)
        rep = f.rep
        if ofv > 3:
            offset = ofv - 3
            rep[:] = [offset, rep[0], rep[1]]
        else:
            idx = ofv + (ll == 0)
            if idx == 1:
                offset = rep[0]
            elif idx == 2:
                offset = rep[1]
                rep[:] = [offset, rep[0], rep[2]]
            else:
                offset = rep[0] - 1 if idx == 4 else rep[2]
                rep[:] = [offset, rep[0], rep[1]]
        need(used + ll <= regen and size() + ll + ml <= limit)
        literals(ll)
        need(offset != 0 and offset <= f.window and offset <= size() - f.start)
        if store:
            at = len(out) - offset
            for k in range(ml):
                out.append(out[at + k])
        else:
            out[0] += ml
    need(bits.left == 0)
    f.have_seq = True
    need(size() + regen - used <= limit)
    literals(regen - used)
    need(size() - start_len <= BLOCK_MAX)


def _payload(p, cap, verify, store):
    """-> (output, status); store False is the MEASURE walk: output is a list of one length."""
    p = bytes(p)
    out = bytearray() if store else [0]

    def size():
        return len(out) if store else out[0]

    pos, st, any_frame = 0, 0, False
    while pos < len(p):
        need(pos + 4 <= len(p))
        magic = struct.unpack_from("<I", p, pos)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            need(pos + 8 <= len(p))
            skip = struct.unpack_from("<I", p, pos + 4)[0]
            need(pos + 8 + skip <= len(p))
            pos += 8 + skip
            continue
        need(magic == 0xFD2FB528 and pos + 5 <= len(p))
        any_frame = True
        fhd = p[pos + 4]
        pos += 5
        fcs_flag, single, checksum = fhd >> 6, bool(fhd & 0x20), bool(fhd & 4)
        did_bytes = (0, 1, 2, 4)[fhd & 3]
        fcs_bytes = (1 if single else 0) if fcs_flag == 0 else 1 << fcs_flag
        need(not fhd & 8 and pos + (0 if single else 1) + did_bytes + fcs_bytes <= len(p))
        window = 0
        if not single:
            wd = p[pos]
            pos += 1
            base = 1 << (10 + (wd >> 3))
            window = base + (base >> 3) * (wd & 7)
        need(not any(p[pos:pos + did_bytes]))
        pos += did_bytes
        fcs = int.from_bytes(p[pos:pos + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0)
        pos += fcs_bytes
        if single:
            window = fcs
        f = Frame(size(), window)
        block_max = min(window, BLOCK_MAX)
        by_fcs = not store and fcs_bytes != 0
        if by_fcs:
            need(fcs <= cap - out[0])
            out[0] += fcs
        while True:
            need(pos + 3 <= len(p))
            bh = p[pos] | (p[pos + 1] << 8) | (p[pos + 2] << 16)
            pos += 3
            kind, bs = (bh >> 1) & 3, bh >> 3
            in_bytes = 1 if kind == 1 else bs
            need(kind != 3 and bs <= block_max and pos + in_bytes <= len(p))
            if not by_fcs:
                limit = min(size() + block_max, cap)
                if kind < 2:
                    need(size() + bs <= limit)
                    if store:
                        out.extend(p[pos:pos + bs] if kind == 0 else p[pos:pos + 1] * bs)
                    else:
                        out[0] += bs
                else:
                    compressed_block(f, p[pos:pos + bs], out, limit, store)
            pos += in_bytes
            if bh & 1:
                break
        if checksum:
            need(pos + 4 <= len(p))
            if store and verify and xxh64(out[f.start:]) & 0xFFFFFFFF != struct.unpack_from("<I", p, pos)[0]:
                st |= CHECKSUM
            pos += 4
        need(by_fcs or fcs_bytes == 0 or fcs == size() - f.start)
    need(any_frame)
    return out, st


def measure(payload):
    """-> (decoded size, status) as the MEASURE kernel reports them."""
    try:
        out, st = _payload(payload, MAX_DECODED, False, False)
    except Corrupt:
        return 0, CORRUPT
    return out[0], st


def decode(payload, verify=True):
    """-> (bytes, status); the bytes are empty unless the status is 0."""
    size, st = measure(payload)
    if st:
        return b"", st
    try:
        out, st = _payload(payload, size, verify, True)
        need(len(out) == size)
    except Corrupt:
        return b"", CORRUPT
    return (bytes(out) if st == 0 else b""), st
