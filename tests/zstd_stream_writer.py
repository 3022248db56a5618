"""Writes Zstandard frames from a PLAN, for the tests of the device decoder (csrc/events_aedat4_zstd.hip states the format): the
test dictates block types, literal modes, stream counts, table modes and the sequences themselves, so every branch of the
decoder can be forced at small sizes.  What tests/aedat4_stream_writer.py is for LZ4.

A plan is a list of blocks: raw(data), rle(byte, count), compressed(literals, sequences, ...).  A sequence is (literal length,
offset value, match length) with the format's Offset_Value: 1..3 are the repeat codes, offset + 3 a new offset.  Writer.frame
returns the frame AND the bytes the plan stands for, from an executor of its own (execute), so a plan cannot be wrong silently.
Nothing here is shared with the decoders under test; the FSE and Huffman tables are derived here from the format's rules.
"""
import heapq
import struct

import aedat4_stream_writer as W

MAGIC = 0xFD2FB528
M64 = (1 << 64) - 1
LL_NORM = [4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4
OF_NORM = [1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5
ML_NORM = [1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7
LL_CODES = [(i, 0) for i in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3), (40, 3), (48, 4), (64, 6)] + \
    [(1 << k, k) for k in range(7, 17)]
ML_CODES = [(i + 3, 0) for i in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3), (67, 4), (83, 4),
                                              (99, 5), (131, 7)] + [((1 << k) + 3, k) for k in range(8, 17)]
PREDEFINED = {"ll": (LL_NORM, 6), "of": (OF_NORM, 5), "ml": (ML_NORM, 6)}
MODES = {"predefined": 0, "rle": 1, "fse": 2, "repeat": 3}


# ------------------------------------------------------------------ XXH64
def xxh64(data, seed=0):
    p1, p2, p3, p4, p5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    rot = lambda v, r: ((v << r) | (v >> (64 - r))) & M64               # noqa: E731
    rnd = lambda a, v: rot((a + v * p2) & M64, 31) * p1 & M64           # noqa: E731
    data = bytes(data)
    n, i = len(data), 0
    if n >= 32:
        acc = [(seed + p1 + p2) & M64, (seed + p2) & M64, seed, (seed - p1) & M64]
        while i + 32 <= n:
            acc = [rnd(a, w) for a, w in zip(acc, struct.unpack_from("<4Q", data, i))]
            i += 32
        h = sum(rot(a, r) for a, r in zip(acc, (1, 7, 12, 18))) & M64
        for a in acc:
            h = ((h ^ rnd(0, a)) * p1 + p4) & M64
    else:
        h = (seed + p5) & M64
    h = (h + n) & M64
    while i + 8 <= n:
        h = (rot(h ^ rnd(0, struct.unpack_from("<Q", data, i)[0]), 27) * p1 + p4) & M64
        i += 8
    if i + 4 <= n:
        h = (rot(h ^ (struct.unpack_from("<I", data, i)[0] * p1 & M64), 23) * p2 + p3) & M64
        i += 4
    for b in data[i:]:
        h = rot(h ^ (b * p5 & M64), 11) * p1 & M64
    h = ((h ^ (h >> 33)) * p2) & M64
    h = ((h ^ (h >> 29)) * p3) & M64
    return h ^ (h >> 32)


# ------------------------------------------------------------------ bit strings
def backward_stream(fields):
    """fields: (value, bits) in the order the decoder READS them -> the bytes, end marker included."""
    total, value = 0, 0
    for v, nb in fields:
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0, (v, nb)
        value = (value << nb) | v
        total += nb
    return ((1 << total) | value).to_bytes(total // 8 + 1, "little")


def forward_stream(fields):
    total, value = 0, 0
    for v, nb in fields:
        assert 0 <= v < (1 << nb)
        value |= v << total
        total += nb
    return value.to_bytes((total + 7) // 8, "little")


# ------------------------------------------------------------------ FSE
def fse_table(norm, log):
    """The decode table of a distribution: (symbol, bits, baseline) per cell."""
    size = 1 << log
    assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
    cells, high = [None] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            cells[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            cells[pos] = s
            pos = (pos + step) % size
            while pos > high:
                pos = (pos + step) % size
    seen = [max(abs(c), 1) for c in norm]
    table = []
    for s in cells:
        nb = log - (seen[s].bit_length() - 1)
        table.append((s, nb, (seen[s] << nb) - size))
        seen[s] += 1
    return table


def fse_description(norm, log):
    """The table description of a distribution, byte-aligned."""
    fields = [(log - 5, 4)]
    remaining, s = 1 << log, 0
    while remaining > 0:
        bits = (remaining + 1).bit_length()
        lower, thresh = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        v = norm[s] + 1
        fields.append((v, bits - 1) if v < thresh else (v, bits) if v <= lower else (v + thresh, bits))
        remaining -= abs(norm[s])
        s += 1
        if norm[s - 1] == 0:
            zeros = 0
            while s < len(norm) and norm[s] == 0:
                zeros += 1
                s += 1
            while zeros >= 3:
                fields.append((3, 2))
                zeros -= 3
            fields.append((zeros, 2))
    assert remaining == 0 and all(c == 0 for c in norm[s:])
    return forward_stream(fields)


def normalize(symbols, log, nsyms):
    """A distribution of accuracy `log` over the symbols used: at least 1 each, the rest by frequency."""
    hist = [0] * nsyms
    for s in symbols:
        hist[s] += 1
    size, total = 1 << log, len(symbols)
    norm = [max(1, c * size // total) if c else 0 for c in hist]
    top = max(range(nsyms), key=lambda s: hist[s])
    norm[top] += size - sum(norm)
    assert norm[top] >= 1, "accuracy %d is too small for these symbols" % log
    while norm and norm[-1] == 0:
        norm.pop()
    return norm


def fse_chain(table, symbols, last_needs_bits=False):
    """The states a decoder walks to emit `symbols` -> (first state, [(bits value, bits) per update])."""
    states = [None] * len(symbols)
    states[-1] = next(u for u, (s, nb, _) in enumerate(table) if s == symbols[-1] and (nb > 0 or not last_needs_bits))
    for i in range(len(symbols) - 2, -1, -1):
        states[i] = next(u for u, (s, nb, base) in enumerate(table) if s == symbols[i] and base <= states[i + 1] < base + (1 << nb))
    return states[0], [(states[i + 1] - table[states[i]][2], table[states[i]][1]) for i in range(len(symbols) - 1)]


# ------------------------------------------------------------------ Huffman
def huffman_weights(literals, limit=11):
    """Weights for the symbols used (at least two): a plain Huffman code; asserts the length limit."""
    hist = {}
    for b in literals:
        hist[b] = hist.get(b, 0) + 1
    assert len(hist) >= 2, "a Huffman tree needs two symbols"
    heap = [(c, s, (s,)) for s, c in hist.items()]
    heapq.heapify(heap)
    depth = dict.fromkeys(hist, 0)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    maxbits = max(depth.values())
    assert maxbits <= limit
    return {s: maxbits + 1 - d for s, d in depth.items()}


def huffman_codes(weights):
    """{symbol: weight} -> ({symbol: (code, bits)}, maxbits) by the decode table's layout."""
    total = sum(1 << (w - 1) for w in weights.values())
    maxbits = total.bit_length() - 1
    assert total == 1 << maxbits, "the weights sum to %d" % total
    codes, cell = {}, 0
    for w in range(1, maxbits + 1):
        for s in sorted(weights):
            if weights[s] == w:
                codes[s] = (cell >> (w - 1), maxbits + 1 - w)
                cell += 1 << (w - 1)
    return codes, maxbits


def huffman_description(weights, how=None, log=6):
    """The tree description: the weights of symbols 0 .. last - 1, the last symbol's is implied.  how: "direct" (at most 128
    weights), "fse"; default: direct where that can be."""
    listed = [weights.get(s, 0) for s in range(max(weights))]
    if (how or ("direct" if len(listed) <= 128 else "fse")) == "direct":
        assert len(listed) <= 128
        padded = listed + [0]
        return bytes([127 + len(listed)]) + bytes((padded[i] << 4) | padded[i + 1] for i in range(0, len(listed), 2))
    assert len(listed) >= 2
    norm = normalize(listed, log, 13)
    table = fse_table(norm, log)
    even, odd = listed[0::2], listed[1::2]
    a_last = len(listed) % 2 == 0                     # the chain that emits the last symbol but one needs bits at its end
    first1, up1 = fse_chain(table, even, last_needs_bits=a_last)
    first2, up2 = fse_chain(table, odd, last_needs_bits=not a_last)
    fields = [(first1, log), (first2, log)]
    for i in range(len(listed) - 2):
        fields.append((up1 if i % 2 == 0 else up2)[i // 2])
    body = fse_description(norm, log) + backward_stream(fields)
    assert len(body) < 128
    return bytes([len(body)]) + body


def huffman_stream(literals, codes):
    return backward_stream([codes[b] for b in literals])


# ------------------------------------------------------------------ blocks
def raw(data):
    return ("raw", bytes(data))


def rle(byte, count):
    return ("rle", byte, count)


def compressed(literals, sequences=(), **how):
    """how: lit="raw" | "rle" | "huffman" | "treeless"; streams=1 | 4; weights={symbol: weight}; tree="direct" | "fse";
    lit_format=size format (Raw / RLE: 0, 1 or 3, where 0 is the one-byte form whose size reaches into bit 3); ll / of / ml = "predefined" | "rle" | "fse" | "repeat"; ll_log / of_log / ml_log; ll_norm / ...;
    tail=bytes that replace the sequence bitstream; cut=bytes dropped from the block's end."""
    return ("compressed", bytes(literals), [tuple(s) for s in sequences], how)


def _code(value, codes):
    k = max(i for i, (base, _) in enumerate(codes) if base <= value)
    return k, value - codes[k][0], codes[k][1]


class Writer:
    """Holds what a frame carries from block to block: the tree for Treeless and the tables for Repeat."""

    def __init__(self):
        self.weights = None
        self.tables = {}

    def literals_section(self, lits, how):
        mode = how.get("lit", "raw")
        fmt = how.get("lit_format")
        n = len(lits)
        if mode in ("raw", "rle"):
            if mode == "rle":
                assert n >= 1 and lits == lits[:1] * n
            if fmt is None:
                fmt = 0 if n < 32 else 1 if n < 4096 else 3
            t = 0 if mode == "raw" else 1
            head = bytes([t | (n << 3)]) if fmt == 0 else \
                struct.pack("<H", t | (fmt << 2) | (n << 4)) if fmt == 1 else struct.pack("<I", t | (fmt << 2) | (n << 4))[:3]
            return head + (lits if mode == "raw" else lits[:1])
        streams = how.get("streams", 1)
        tree = b""
        if mode == "huffman":
            self.weights = how.get("weights") or huffman_weights(lits)
            tree = how.get("tree_bytes") or huffman_description(self.weights, how.get("tree"), how.get("tree_log", 6))
        codes, _ = huffman_codes(self.weights) if how.get("check_weights", True) else ({}, 0)
        if streams == 1:
            body = huffman_stream(lits, codes)
        else:
            each = (n + 3) // 4
            parts = [huffman_stream(lits[k * each:(k + 1) * each], codes) for k in range(4)]
            body = struct.pack("<3H", *(len(p) for p in parts[:3])) + b"".join(parts)
        comp = len(tree) + len(body)
        if fmt is None:
            fmt = 0 if streams == 1 else 1 if max(n, comp) < 1024 else 2 if max(n, comp) < 16384 else 3
        assert (fmt == 0) == (streams == 1)
        nb = 10 if fmt < 2 else 14 if fmt == 2 else 18
        assert n < (1 << nb) and comp < (1 << nb)
        t = 2 if mode == "huffman" else 3
        v = t | (fmt << 2) | (n << 4) | (comp << (4 + nb))
        return v.to_bytes(3 if fmt < 2 else fmt + 2, "little") + tree + body

    def table(self, kind, symbols, nsyms, how):
        """-> (mode, the bytes that describe the table, the table, its accuracy)"""
        mode = how.get(kind, "predefined")
        if mode == "predefined":
            norm, log = PREDEFINED[kind]
            self.tables[kind] = (fse_table(norm, log), log)
            return 0, b""
        if mode == "rle":
            assert len(set(symbols)) == 1
            self.tables[kind] = ([(symbols[0], 0, 0)], 0)
            return 1, bytes([how.get(kind + "_symbol", symbols[0])])
        if mode == "fse":
            log = how.get(kind + "_log", 6)
            norm = how.get(kind + "_norm") or normalize(symbols, log, nsyms)
            self.tables[kind] = (fse_table(norm, log), log)
            return 2, fse_description(norm, log)
        assert mode == "repeat"
        return 3, b""

    def sequences_section(self, seqs, how):
        n = len(seqs)
        count = how.get("count_bytes") or (bytes([n]) if n < 128 else bytes([128 + (n >> 8), n & 255]) if n < 0x7F00 else
                                           b"\xff" + struct.pack("<H", n - 0x7F00))
        if n == 0:
            return count
        ll = [_code(s[0], LL_CODES) for s in seqs]
        of = [(s[1].bit_length() - 1, s[1] - (1 << (s[1].bit_length() - 1)), s[1].bit_length() - 1) for s in seqs]
        ml = [_code(s[2], ML_CODES) for s in seqs]
        modes, described = 0, b""
        for kind, codes, nsyms, shift in (("ll", ll, 36, 6), ("of", of, 32, 4), ("ml", ml, 53, 2)):
            m, d = self.table(kind, [c[0] for c in codes], nsyms, how)
            modes |= m << shift
            described += d
        if "tail" in how:
            return count + bytes([modes | how.get("reserved_modes", 0)]) + described + how["tail"]
        chains = {}
        for kind, codes in (("ll", ll), ("of", of), ("ml", ml)):
            table, log = self.tables[kind]
            first, ups = fse_chain(table, [c[0] for c in codes])
            chains[kind] = ((first, log), ups)
        fields = [chains["ll"][0], chains["of"][0], chains["ml"][0]]
        for i in range(n):
            fields += [of[i][1:], ml[i][1:], ll[i][1:]]
            if i + 1 < n:
                fields += [chains["ll"][1][i], chains["ml"][1][i], chains["of"][1][i]]
        return count + bytes([modes | how.get("reserved_modes", 0)]) + described + backward_stream(fields)

    def block(self, plan, last):
        kind = plan[0]
        if kind == "raw":
            body, t, size = plan[1], 0, len(plan[1])
        elif kind == "rle":
            body, t, size = bytes([plan[1]]), 1, plan[2]
        elif kind == "bytes":                         # ("bytes", type, size field, the bytes): anything at all
            t, size, body = plan[1], plan[2], plan[3]
        else:
            how = plan[3]
            body = self.literals_section(plan[1], how) + self.sequences_section(plan[2], how)
            if how.get("cut"):
                body = body[:-how["cut"]]
            t, size = 2, len(body)
        return struct.pack("<I", int(last) | (t << 1) | (size << 3))[:3] + body

    def frame(self, blocks, checksum=False, single=False, fcs_bytes=None, window=0x38, did=None, descriptor_or=0, fcs=None,
              magic=MAGIC, bad_checksum=False):
        """-> (the frame, the bytes its plan stands for).  window: the descriptor byte (0x38: 128 KiB; 0: 1 KiB).  fcs_bytes: 0, 1
        (single segment only), 2, 4, 8; default 0, or the smallest that fits when single.  did: the bytes of a dictionary ID field."""
        data = execute(blocks)
        n = len(data) if fcs is None else fcs
        if fcs_bytes is None:
            fcs_bytes = 0 if not single else 1 if n < 256 else 2 if n < 65536 + 256 else 4
        assert fcs_bytes != 1 or single
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
        did = did or b""
        head = bytes([(flag << 6) | (0x20 if single else 0) | (4 if checksum else 0) | {0: 0, 1: 1, 2: 2, 4: 3}[len(did)] | descriptor_or])
        if not single:
            head += bytes([window])
        head += did
        if fcs_bytes:
            head += (n - 256 if fcs_bytes == 2 else n).to_bytes(fcs_bytes, "little")
        out = struct.pack("<I", magic) + head
        for k, plan in enumerate(blocks):
            out += self.block(plan, k == len(blocks) - 1)
        if checksum:
            out += struct.pack("<I", (xxh64(data) & 0xFFFFFFFF) ^ (0x5A5A if bad_checksum else 0))
        return out, data


def frame(blocks, **kw):
    return Writer().frame(blocks, **kw)


def skippable(payload=b"skip me", nibble=0):
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload)) + payload


def advance(rep, ofv, ll):
    """The repeat offsets after a sequence of offset value ofv and literal length ll; the sequence's offset is the first."""
    if ofv > 3:
        return [ofv - 3, rep[0], rep[1]]
    k = ofv + (ll == 0)
    return rep if k == 1 else [rep[1], rep[0], rep[2]] if k == 2 else [rep[2] if k == 3 else rep[0] - 1, rep[0], rep[1]]


def execute(blocks):
    """The bytes a plan stands for."""
    out, rep = bytearray(), [1, 4, 8]
    for plan in blocks:
        if plan[0] == "raw":
            out += plan[1]
        elif plan[0] == "rle":
            out += bytes([plan[1]]) * plan[2]
        elif plan[0] == "compressed":
            lits, at = plan[1], 0
            for ll, ofv, ml in plan[2]:
                out += lits[at:at + ll]
                at += ll
                rep = advance(rep, ofv, ll)
                if plan[3].get("execute", True):            # False: a plan that is damaged on purpose
                    assert 0 < rep[0] <= len(out), "offset %d after %d bytes" % (rep[0], len(out))
                    for _ in range(ml):
                        out.append(out[-rep[0]])
            out += lits[at:]
    return bytes(out)


# ------------------------------------------------------------------ recordings
def write_aedat4(packets, streams, compress, compression=W.ZSTD, **kw):
    """W.write_aedat4 of ZSTD payloads: payload k becomes compress(k, payload), the header says `compression` (3 or 4)."""
    return W.write_aedat4([(sid, compress(k, payload)) for k, (sid, payload) in enumerate(packets)], streams, compression, **kw)


def greedy_plan(data, block=1 << 17, min_match=4, **how):
    """data as Compressed blocks of at most `block` bytes: a greedy matcher on a hash of 4 bytes, offsets reaching back into
    earlier blocks; an offset that is the first or second repeat offset is written as its repeat code, any other as a new offset
    (value offset + 3).  The repeat offsets run on from block to block, as the format has it."""
    data = bytes(data)
    seen, blocks, rep = {}, [], [1, 4, 8]
    for start in range(0, len(data), block):
        end = min(start + block, len(data))
        lits, seqs, i, run = bytearray(), [], start, start
        while i + min_match <= end:
            key = data[i:i + 4]
            j = seen.get(key)
            seen[key] = i
            r = rep[0 if i > run else 1]              # the offset that costs least here, if it matches
            if i - r >= 0 and data[i - r:i - r + 4] == key:
                j = i - r
            if j is not None:
                n = 4
                while i + n < end and data[i + n] == data[j + n]:
                    n += 1
                lits += data[run:i]
                ll, off = i - run, i - j
                ofv = 1 if off == rep[0 if ll else 1] else 2 if ll and off == rep[1] else off + 3
                rep = advance(rep, ofv, ll)
                assert rep[0] == off
                seqs.append((ll, ofv, n))
                i += n
                run = i
            else:
                i += 1
        lits += data[run:end]
        blocks.append(compressed(bytes(lits), seqs, **how))
    return blocks or [raw(b"")]
