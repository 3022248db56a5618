"""The files of tests/test_jpeg_streams.py and tests/test_gpu_jpeg_streams.py: baseline JPEG streams that no PIL encoder
writes, made at test time by tests/jpeg_stream_writer.py from seeds and by construction.  Every family is a list of Case."""
import functools

import numpy as np

import jpeg_decode_restated as R
import jpeg_stream_writer as W

J, S = R.J, R.S
ZZ = np.array(W.ZIGZAG)

# ---- tables.  T.81 table K.3 (luminance DC), then tables of this file's own
DC_K3 = W.dc_table([2, 3, 3, 3, 3, 3, 4, 5, 6, 7, 8, 9])
DC_LONG = W.dc_table([13, 13, 13, 14, 14, 14, 15, 15, 15, 16, 16, 16])            # every code 13 .. 16 bits
DC_MID = W.dc_table([2, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11])
AC_EDGE = W.ac_table({0x00: 2, 0x01: 3, 0x11: 4, 0x21: 5, 0xF0: 6, 0x02: 9, 0x03: 10})     # 9 and 10 bits: the first-level edge
AC_B = W.ac_table({0x01: 2, 0x00: 3, 0x02: 3, 0x11: 5, 0x03: 5, 0x04: 6, 0x21: 7, 0x31: 8, 0xF0: 9}, rest=15)
AC_C = W.ac_table({0x01: 2, 0x02: 2, 0x03: 3, 0x00: 4, 0x11: 4, 0x12: 5, 0x21: 6, 0xF0: 7}, rest=14)
DC_TABLES = {2: DC_LONG, 0: DC_MID, 3: DC_K3}
AC_TABLES = {2: AC_EDGE, 3: AC_B, 0: AC_C}
IDS = dict(comp_ids=[7, 9, 200], comp_q=[2, 0, 3], comp_dc=[2, 0, 3], comp_ac=[2, 3, 0])
GRAY_IDS = dict(comp_ids=[7], comp_q=[2], comp_dc=[2], comp_ac=[2])


class Case:
    def __init__(self, name, data, written=None, **kw):
        self.name, self.data, self.written = name, data, written
        self.__dict__.update(kw)

    @functools.cached_property
    def stream(self):
        return R.Stream(self.data)

    @functools.cached_property
    def sequential(self):
        return R.decode_sequential(self.stream)

    @functools.cached_property
    def relaxed(self):
        return R.relax(self.stream)

    @functools.cached_property
    def pil(self):
        return R.pil_decode(self.data)

    @property
    def geometry(self):
        return self.stream.h.geometry


def n_blocks(h, w, mode):
    m = 16 if mode == "420" else 8
    return -(-h // m) * -(-w // m) * {"gray": 1, "444": 3, "420": 6}[mode]


def qtables(seed, top=(9, 13, 6)):
    rng = np.random.default_rng(1000 + seed)
    return {t: rng.integers(1, hi, 64) for t, hi in zip((2, 0, 3), top)}


def sparse_blocks(rng, n, dc_span=60, density=0.08, amp=7):
    """n blocks, zig-zag order: a DC value and a few small AC coefficients anywhere up to index 63"""
    b = np.zeros((n, 64), dtype=np.int64)
    b[:, 0] = rng.integers(-dc_span, dc_span + 1, n)
    b[:, 1:] = (rng.random((n, 63)) < density) * rng.integers(1, amp + 1, (n, 63)) * rng.choice([-1, 1], (n, 63))
    return b


def colour(h, w, mode, blocks, seed=0, ri=0, **kw):
    ids = GRAY_IDS if mode == "gray" else IDS
    return W.write(h, w, mode, blocks, kw.pop("q", None) or qtables(seed), DC_TABLES, AC_TABLES, restart_interval=ri, **ids, **kw)


def prelimit_range(case):
    """(min, max) of the exact ISLOW output before + 128 and the range limit, over every block of the file"""
    st = case.stream
    coef, _ = case.sequential
    h = st.h
    lo, hi = 0, 0
    nb = coef.reshape(h.n_mcus, st.bpm, 64)
    for c in range(h.ncomp):
        first, cnt = (0, h.hmax * h.vmax) if c == 0 else (h.hmax * h.vmax + c - 1, 1)
        x = (nb[:, first:first + cnt].reshape(-1, 64).astype(np.int64) * h.qt[h.comp_q[c]].astype(np.int64)[None, :]).reshape(-1, 8, 8)
        ws = R._pass(x.transpose(0, 2, 1), 13 - 2, 13).transpose(0, 2, 1)
        out = R._pass(ws, 13 + 2 + 3, 13)
        lo, hi = min(lo, int(out.min())), max(hi, int(out.max()))
    return lo, hi


# ------------------------------------------------------------------ A: tables per component
@functools.lru_cache(None)
def family_a():
    cases = []
    for mode, (h, w) in (("444", (16, 17)), ("420", (33, 31)), ("gray", (16, 17))):
        for ri in (0, 1, 3):
            rng = np.random.default_rng(100 * h + 10 * w + ri)
            b = sparse_blocks(rng, n_blocks(h, w, mode), density=0.2)
            b[:, 0] = rng.choice([0, 1, -1, 2, -2, 3, -5, 9, -20, 40, -90, 200, -280, 270], len(b))   # differences of every size up to 10
            data, wr = colour(h, w, mode, b, seed=1, ri=ri)
            cases.append(Case("A-%s-%dx%d-ri%d" % (mode, h, w, ri), data, wr))
    return cases


# ------------------------------------------------------------------ B: geometry
B_SIZES = ((1, 1), (2, 3), (3, 4), (1, 5), (2, 6), (3, 37), (16, 17), (33, 31), (5, 261), (4, 260), (9, 515))


@functools.lru_cache(None)
def family_b(mode):
    cases = []
    for h, w in B_SIZES:
        for ri in (0, 1, 3):
            rng = np.random.default_rng(7 * h + w + ri)
            data, wr = colour(h, w, mode, sparse_blocks(rng, n_blocks(h, w, mode)), seed=h + w, ri=ri)
            cases.append(Case("B-%s-%dx%d-ri%d" % (mode, h, w, ri), data, wr))
        cases.append(Case("B-%s-%dx%d-pil" % (mode, h, w), R.fixture(mode, h, w, 90, "noise", seed=h)))
    return cases


# ------------------------------------------------------------------ C: segment ends
Q1 = {t: np.ones(64, dtype=np.int64) for t in range(4)}


def gray(h, w, blocks, ri=0, dc=DC_K3, ac=AC_C, ids=(1, 0, 0, 0)):
    return W.write(h, w, "gray", blocks, Q1, {ids[2]: dc}, {ids[3]: ac}, comp_ids=[ids[0]], comp_q=[ids[1]], comp_dc=[ids[2]],
                   comp_ac=[ids[3]], restart_interval=ri)


def block_to_63(v):
    """DC 0, then nothing but a coefficient at index 63: three ZRL and a run of 14, and no EOB"""
    b = np.zeros(64, dtype=np.int64)
    b[63] = v
    return b


@functools.lru_cache(None)
def family_c():
    cases, found = [], {}
    for nblk in (1, 2):                                                   # a free DC value, then a second coefficient too
        seen = {}
        for second in (0, 1, -2, 5, -11, 23, 40):
            for dcv in range(-200, 200):
                b = np.zeros((nblk, 64), dtype=np.int64)
                b[-1, 0], b[-1, 5] = dcv, second
                b[0, 0] += 3 * (nblk - 1)
                data, wr = gray(8, 8 * nblk, b)
                if wr.fill_bits[0] not in seen:
                    seen[wr.fill_bits[0]] = Case("C-%dblk-fill%d" % (nblk, wr.fill_bits[0]), data, wr, fills=set(wr.fill_bits), blocks=b)
            if len(seen) == 8:
                break
        cases += [seen[k] for k in sorted(seen)]
        found[nblk] = seen
    # a segment whose last data byte is FF: the block ends at index 63 on value bits of ones, the fill bits are ones
    for v in (255, 1023):
        data, wr = gray(8, 8, block_to_63(v)[None])
        cases.append(Case("C-last-byte-ff-%d" % v, data, wr, fills=set(wr.fill_bits), last_ff=True))
    # restart interval 1 over 10 MCUs: RST0 .. RST7, RST0 again; the blocks are the swept ones, one per fill count, and the FF one
    one = found[1]
    blocks = np.zeros((10, 64), dtype=np.int64)
    for i in range(8):
        blocks[i] = one[i].blocks[0]
    blocks[8] = block_to_63(255)
    blocks[9] = blocks[3]
    data, wr = gray(8, 80, blocks, ri=1)
    cases.append(Case("C-ri1-10-segments", data, wr, fills=set(wr.fill_bits), wraps=True))
    return cases


# ------------------------------------------------------------------ D: subsequence boundaries, by construction
DC_D = W.dc_table([2, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16])                # size 11: 16 + 11 = 27 bits, the longest code word
AC_D = W.ac_table({0x00: 2, 0x01: 2, 0x0A: 3})                            # (0, 10) with value 1023: ten one bits
D_H, D_W, D_BOUNDS = 64, 80, 8


def raw_boundary_bit(data_bytes, raw_index):
    """data bit at which raw byte `raw_index` starts (one byte later when it is a stuffed zero), as Segment.bound counts"""
    raw = 0
    for j, c in enumerate(data_bytes):
        if raw >= raw_index:
            return 8 * j
        raw += 2 if c == 0xFF else 1
    return 8 * len(data_bytes)


class Builder:
    """blocks appended one by one with the bit position known, so that a chosen code word lands on a chosen bit"""

    def __init__(self):
        self.blocks, self.out, self.dc = [], W.Bits(), 0
        self.dcc, self.acc = W.codes(DC_D), W.codes(AC_D)

    def add(self, diff, ac=()):
        b = np.zeros(64, dtype=np.int64)
        b[0] = self.dc + diff
        b[1:1 + len(ac)] = ac
        W.code_block(self.out, b, self.dc, self.dcc, self.acc, set(), set())
        self.dc += diff
        self.blocks.append(b)

    def filler(self, n, one):
        """2 (+ 1) bits of DC, 3 bits per +-1 coefficient, 2 bits of EOB"""
        self.add((-1 if self.dc > 0 else 1) if one else 0, [1 - 2 * (i & 1) for i in range(n)])

    def fill_to(self, target):
        while target - self.out.n > 320:
            self.filler(56, False)
        r = target - self.out.n - 8
        assert r >= 0, "no room before bit %d" % target
        e, n = r % 3, r // 3
        self.filler(n // 2, e >= 1)
        self.filler(n - n // 2, e >= 2)
        assert self.out.n == target

    def clone(self):
        t = Builder()
        t.blocks, t.dc, t.out.acc, t.out.n = list(self.blocks), self.dc, self.out.acc, self.out.n
        return t

    def data_bytes(self):
        pad = -self.out.n % 8
        return (((self.out.acc << pad) | ((1 << pad) - 1)).to_bytes((self.out.n + pad) // 8, "big"))

    def stuffed_before(self):
        return self.data_bytes()[:self.out.n // 8].count(0xFF)


def build_d(targets):
    """targets: per boundary i = 1 .. either ('d', overhang) or ('ff', 0 | 1: the FF is raw byte i * S - 1 | i * S)"""
    b = Builder()
    b.add(-515)
    for i, (kind, arg) in enumerate(targets, start=1):
        for extra in (0, 1):                       # the long code word may itself hold an FF before the boundary: one stuffed byte more
            t = b.clone()
            base = 8 * (i * S - t.stuffed_before() - extra)
            if kind == "d":
                t.fill_to(base + arg - 27)
                end = t.out.n + 27
                t.add(-1030 if t.dc > 0 else 1030)
                ok = end - raw_boundary_bit(t.data_bytes(), i * S) == arg
            else:
                t.fill_to(base - 8 * (1 - arg) - 6)
                t.add(0, [1023])
                raw = t.data_bytes().replace(b"\xff", b"\xff\x00")
                ok = raw[i * S - 1 + arg] == 0xFF and raw[i * S + arg] == 0
            if ok:
                break
        assert ok, (i, kind, arg)
        b = t
    total = n_blocks(D_H, D_W, "gray")
    assert len(b.blocks) <= total, len(b.blocks)
    while len(b.blocks) < total:
        b.filler(0, False)
    return W.write(D_H, D_W, "gray", np.stack(b.blocks), Q1, {1: DC_D}, {1: AC_D}, comp_ids=[1], comp_q=[0], comp_dc=[1], comp_ac=[1])


@functools.lru_cache(None)
def family_d():
    targets = [("d", d) for d in range(27)] + [("ff", 0), ("ff", 1)]
    targets = targets[0::4] + targets[1::4] + targets[2::4] + targets[3::4]       # small and large overhangs in every file
    cases = []
    for k in range(0, len(targets), D_BOUNDS):
        data, wr = build_d(targets[k:k + D_BOUNDS])
        cases.append(Case("D-%d" % (k // D_BOUNDS), data, wr, targets=targets[k:k + D_BOUNDS]))
    return cases


# ------------------------------------------------------------------ E: runs and extremes inside a block
DC_SHORT = W.dc_table([1, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])            # no difference: one bit
AC_EOB1 = W.ac_table({0x00: 1, 0x01: 3})
AC_EOB2 = W.ac_table({0x00: 2, 0x01: 2, 0x02: 3})


@functools.lru_cache(None)
def family_e():
    cases = []
    # three ZRL and a coefficient at index 63, no EOB; then the same with an EOB-ended block before and after
    b = np.zeros((4, 64), dtype=np.int64)
    b[0] = block_to_63(-3); b[1, 0] = 9; b[2] = block_to_63(77); b[2, 0] = -20; b[3, 0] = 9; b[3, 1:] = 1     # [3]: 63 coefficients
    data, wr = gray(16, 16, b, ids=(5, 1, 3, 2), dc=DC_MID)
    cases.append(Case("E-zrl-to-63", data, wr, zrl=True))
    # hundreds of all-zero blocks in one subsequence: EOB of one bit (gray) and of two bits (4:2:0, the block cycle wraps)
    z = np.zeros((n_blocks(256, 256, "gray"), 64), dtype=np.int64)
    z[0, 0], z[700, 0], z[701, 0] = 5, 5, -7
    data, wr = W.write(256, 256, "gray", z, Q1, {0: DC_SHORT}, {0: AC_EOB1})
    cases.append(Case("E-eob1-gray", data, wr, zeros=True))
    z = np.zeros((n_blocks(128, 256, "420"), 64), dtype=np.int64)
    z[0, 0], z[4, 0], z[5, 0], z[602, 0], z[603, 1] = 5, -30, 30, 9, 1
    data, wr = W.write(128, 256, "420", z, Q1, {0: DC_SHORT, 1: DC_K3}, {0: AC_EOB2, 1: AC_EOB1}, comp_dc=[0, 1, 0], comp_ac=[0, 1, 1])
    cases.append(Case("E-eob2-420", data, wr, zeros=True))
    # the extremes of the format: AC +-1023, DC differences +-2047 (the DC value swings between -1024 and 1023)
    for mode in ("gray", "420"):
        n = n_blocks(16, 32, mode)
        x = np.zeros((n, 64), dtype=np.int64)
        pos = np.arange(n) % (1 if mode == "gray" else 6)
        comp = np.where(pos < 4, 0, pos - 3)
        for c in set(comp.tolist()):
            mine = np.flatnonzero(comp == c)
            x[mine[0::2], 0], x[mine[1::2], 0] = -1024, 1023
        x[0, 1], x[1, 2], x[n - 1, 63], x[n - 2, 7] = 1023, -1023, -1023, 1023
        data, wr = colour(16, 32, mode, x, q=Q1)
        cases.append(Case("E-extremes-%s" % mode, data, wr, extremes=True, blocks=x))
    return cases


# ------------------------------------------------------------------ F: saturation and colour
CUBE = (0, 1, 64, 127, 128, 129, 200, 254, 255)


@functools.lru_cache(None)
def family_f():
    cases = [Case("F-pil-%s-q%d" % (mode, q), R.fixture(mode, 48, 40, q, "noise")) for mode in ("gray", "420") for q in (1, 5, 10)]
    # 729 flat patches: (dc + 4) >> 3 is the sample minus 128, so dc = 8 (v - 128) gives v
    ycc = np.array([(y, cb, cr) for y in CUBE for cb in CUBE for cr in CUBE])
    x = np.zeros((729, 3, 64), dtype=np.int64)
    x[:, :, 0] = 8 * (ycc - 128)
    data, wr = colour(216, 216, "444", x.reshape(-1, 64), q=Q1)
    cases.append(Case("F-cube-444", data, wr, cube=True))
    # 4:2:0: flat luma from the same values, chroma that alternates from sample to sample (the highest frequencies, saturated)
    rng = np.random.default_rng(5)
    n_mcu = 9
    x = np.zeros((n_mcu, 6, 64), dtype=np.int64)
    x[:, :4, 0] = 8 * (rng.choice(CUBE, (n_mcu, 4)) - 128)
    x[:, 4:, 0] = 8 * (rng.choice(CUBE, (n_mcu, 2)) - 128)
    x[:, 4, 63], x[:, 5, 28], x[:, 5, 35] = rng.choice([-900, 900], n_mcu), rng.choice([-700, 700], n_mcu), rng.choice([-700, 700], n_mcu)
    x[4, 4:, 1:] = 0                                                      # one MCU of flat chroma between the others
    data, wr = colour(48, 48, "420", x.reshape(-1, 64), q=Q1, ri=2)
    cases.append(Case("F-steps-420", data, wr, steps=True))
    return cases


# ------------------------------------------------------------------ G: the relaxation's worst case
G_H, G_W = 128, 192


@functools.lru_cache(None)
def family_g():
    # periodic content: every block the same 63 small coefficients, so a walk from a wrong state never meets a landmark
    rng = np.random.default_rng(11)
    one = np.zeros(64, dtype=np.int64)
    one[1:] = rng.integers(1, 4, 63) * rng.choice([-1, 1], 63)
    n = n_blocks(G_H, G_W, "gray")
    data, wr = gray(G_H, G_W, np.tile(one, (n, 1)), dc=DC_MID, ac=AC_B, ids=(1, 1, 1, 1))
    easy, _ = gray(G_H, G_W, np.zeros((n, 64), dtype=np.int64), dc=DC_SHORT, ac=AC_EOB1)
    wide = R.fixture("gray", 144, 144, 100, "noise", seed=2, restart_marker_blocks=9)
    return [Case("G-periodic", data, wr, periodic=True), Case("G-one-round", easy), Case("G-sub256", wide, wide=True)]



def cpu_families():
    return {"A": family_a(), "B": [c for m in ("gray", "444", "420") for c in family_b(m)], "C": family_c(), "D": family_d(),
            "E": family_e(), "F": family_f(), "G": family_g()}
