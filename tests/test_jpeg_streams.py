"""Baseline JPEG streams that no PIL encoder writes (tests/jpeg_stream_families.py, written by tests/jpeg_stream_writer.py),
without a device: for every file the restatement equals PIL bit for bit, the relaxation converges to the sequential decode's
entry states in at most as many rounds as the file has subsequences, and every family shows from the bytes, the writer's record
and the states that it holds the case it was made for."""
import numpy as np
import pytest

import jpeg_decode_restated as R
import jpeg_stream_families as F
import jpeg_stream_writer as W

J, S = R.J, R.S


def check(case):
    """the three assertions every file of every family gets -> rounds"""
    st = case.stream
    coef, states = case.sequential
    assert np.array_equal(R.render(st, coef), case.pil), case.name
    assert np.array_equal(R.render(st, coef, rgb=False), case.pil[:, :, ::-1]), case.name
    entries, rounds, converged = case.relaxed
    assert converged and entries == states, case.name
    assert 1 <= rounds <= st.h.nsub, (case.name, rounds, st.h.nsub)       # never more rounds than subsequences
    if case.written is not None:                                          # the parser finds the segments the writer wrote
        assert [bytes(st.data[a:b]) for a, b in zip(st.h.seg_start, st.h.seg_end)] == case.written.entropy, case.name
        assert [8 * len(e.replace(b"\xff\x00", b"\xff")) for e in case.written.entropy] == \
            [d + f for d, f in zip(case.written.data_bits, case.written.fill_bits)]
    return rounds


def in_window(case):
    lo, hi = F.prelimit_range(case)
    assert -512 <= lo and hi <= 511, (case.name, lo, hi)                  # outside it libjpeg's C and SIMD range limits part ways
    return lo, hi


def test_writer_tables_follow_annex_c():
    """the code assignment of T.81 annex C on table K.3, and the value bits of F.1.2.1.1"""
    c = W.codes(F.DC_K3)
    assert [c[s] for s in range(12)] == [(0, 2), (2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (14, 4), (30, 5), (62, 6), (126, 7), (254, 8), (510, 9)]
    assert [(W.size_of(v), W.value_bits(v, W.size_of(v))) for v in (0, 1, -1, 2, -3, 1023, -1023, 2047, -2047)] == \
        [(0, 0), (1, 1), (1, 0), (2, 2), (2, 0), (10, 1023), (10, 0), (11, 2047), (11, 0)]
    for tab in (F.DC_LONG, F.AC_EDGE, F.AC_B, F.AC_C, F.DC_D, F.AC_D, F.AC_EOB1):
        bits, vals = tab
        code, l = max(W.codes(tab).values(), key=lambda cl: (cl[1], cl[0]))
        assert sum(bits) == len(vals) == len(set(vals)) and code != (1 << l) - 1     # no code of ones only


def test_a_tables_per_component():
    lengths = {"dc": set(), "ac": set()}
    for case in F.family_a():
        check(case)
        in_window(case)
        h, wr = case.stream.h, case.written
        if h.ncomp == 3:
            assert (h.comp_q, h.comp_dc, h.comp_ac) == ([2, 0, 3], [2, 0, 3], [2, 3, 0])
            assert len({h.qt[t].tobytes() for t in h.comp_q}) == 3
            assert len({h.dc_huffval[t].tobytes() + h.dc_bits[t].tobytes() for t in h.comp_dc}) == 3
            assert len({h.ac_huffval[t].tobytes() + h.ac_bits[t].tobytes() for t in h.comp_ac}) == 3
            # what a kernel that took Cr's tables from Cb would read: another descriptor, and with q[2] = q[1] another picture
            d = J.descriptor(h)
            slot = lambda i: d[J.DESC_TABLES_OFF + i * J.SLOT_BYTES:J.DESC_TABLES_OFF + (i + 1) * J.SLOT_BYTES].tobytes()
            q = d[J.DESC_QUANT_OFF:J.DESC_TABLES_OFF].view(np.uint16).reshape(3, 64)
            assert slot(4) != slot(2) and slot(5) != slot(3) and slot(2) != slot(0) and slot(3) != slot(1)
            assert not np.array_equal(q[2], q[1]) and not np.array_equal(q[1], q[0])
            shared = R.Stream(case.data)
            shared.h.comp_q = [h.comp_q[0], h.comp_q[1], h.comp_q[1]]
            assert not np.array_equal(R.render(shared, case.sequential[0]), case.pil), case.name
            shared = R.Stream(case.data)
            shared.dc[2], shared.ac[2] = shared.dc[1], shared.ac[1]
            try:
                differs = not np.array_equal(R.render(shared, R.decode_sequential(shared)[0]), case.pil)
            except J.JpegError:
                differs = True
            assert differs, case.name
        else:
            assert (h.comp_q, h.comp_dc, h.comp_ac) == ([2], [2], [2])                # a gray file whose table ids are not 0
        assert wr.dc_lengths[2] and wr.dc_lengths[2] <= {13, 14, 15, 16}         # the DC table of 13 .. 16 bits
        assert {9, 10, 16} <= wr.ac_lengths[2], wr.ac_lengths[2]                       # both sides of the first-level table
        lengths["dc"] |= wr.dc_lengths[2]; lengths["ac"] |= wr.ac_lengths[2]
    assert lengths["dc"] == {13, 14, 15, 16}
    assert {c.stream.h.restart_interval for c in F.family_a()} == {0, 1, 3}
    print("A: code lengths emitted, luma DC %s, luma AC %s" % (sorted(lengths["dc"]), sorted(lengths["ac"])))


@pytest.mark.parametrize("mode", ("gray", "444", "420"))
def test_b_geometry(mode):
    cases = F.family_b(mode)
    for case in cases:
        check(case)
        if case.written is not None:
            in_window(case)
    sizes = {c.stream.h.geometry[:2] for c in cases}
    assert sizes == set(F.B_SIZES)
    dw, dh = {(w + 1) // 2 for _, w in sizes}, {(h + 1) // 2 for h, _ in sizes}
    assert {1, 2, 3} <= dw and {1, 2} <= dh
    assert any(w > 256 and w % 4 for _, w in sizes) and any(w > 256 and w % 4 == 0 for _, w in sizes) and any(w > 512 for _, w in sizes)
    print("B %s: %d files, sizes %s" % (mode, len(cases), sorted(sizes)))


def test_c_segment_ends():
    cases = F.family_c()
    for case in cases:
        check(case)
        in_window(case)
    for nblk in (1, 2):
        fills = set()
        for c in cases:
            if c.name.startswith("C-%dblk" % nblk):
                assert c.stream.h.n_blocks == nblk
                fills |= c.fills
        assert fills == set(range(8)), (nblk, fills)
    ff = [c for c in cases if getattr(c, "last_ff", False)]
    assert ff and all(c.written.entropy[0].endswith(b"\xff\x00") for c in ff)          # the stuffed zero is the last raw byte
    wrap, = [c for c in cases if getattr(c, "wraps", False)]
    h = wrap.stream.h
    assert h.restart_interval == 1 and h.seg_start.size >= 9
    marks = [wrap.data[e + 1] for e in h.seg_end[:-1].tolist()]
    assert marks[:9] == [0xD0 + i for i in range(8)] + [0xD0]                          # RST7, then RST0 again
    assert len(wrap.fills) >= 4 and any(e.endswith(b"\xff\x00") for e in wrap.written.entropy)
    print("C: fill bits %s in one-block files, %s in the %d-segment file" % (sorted(fills), sorted(wrap.fills), h.seg_start.size))


def test_d_subsequence_boundaries():
    overhangs, zero_at, ff_at = set(), 0, 0
    for case in F.family_d():
        check(case)
        in_window(case)
        h = case.stream.h
        assert h.seg_start.size == 1 and h.nsub > 4
        body = case.data[h.data_start:h.data_end]
        states, = case.sequential[1]
        for i, (kind, arg) in enumerate(case.targets, start=1):
            if kind == "d":
                assert states[i][0] == arg, (case.name, i, states[i])
            elif arg == 0:
                assert body[i * S - 1] == 0xFF and body[i * S] == 0
                zero_at += 1
            else:
                assert body[i * S] == 0xFF and body[i * S + 1] == 0
                ff_at += 1
        overhangs |= {s[0] for s in states[1:]}
        assert 16 in case.written.dc_lengths[1]                                        # the 16-bit DC code and its 11 value bits
    assert set(range(27)) <= overhangs and max(overhangs) == 26, sorted(overhangs)
    assert zero_at >= 1 and ff_at >= 1
    print("D: overhangs %s; stuffed zero on a boundary %d, FF on a boundary %d" % (sorted(overhangs), zero_at, ff_at))


def test_e_runs_and_extremes():
    for case in F.family_e():
        check(case)
        lo, hi = in_window(case)
        st, wr = case.stream, case.written
        if getattr(case, "zrl", False):
            coef = case.sequential[0]
            raw = wr.entropy[0]
            assert coef[0, 63] == -3 and not coef[0, :63].any() and coef[2, 63] == 77 and np.count_nonzero(coef[3]) == 64
            zrl, zl = W.codes(F.AC_C)[0xF0]
            bits = bin(int.from_bytes(raw.replace(b"\xff\x00", b"\xff"), "big"))[2:].zfill(8 * len(raw))
            assert bits[2:].startswith(format(zrl, "0%db" % zl) * 3)                   # DC size 0 (2 bits), then three ZRL
        if getattr(case, "zeros", False):
            most = max(st.run(seg, i, e)[1] for seg, ent in zip(st.segs, case.sequential[1]) for i, e in enumerate(ent))
            assert most >= 200 and most > 30 * st.bpm, most
            print("E %s: %d blocks completed by one subsequence" % (case.name, most))
        if getattr(case, "extremes", False):
            b = case.blocks
            assert b[:, 1:].max() == 1023 and b[:, 1:].min() == -1023
            diffs = set()
            for c in range(st.h.ncomp):
                dcs = b[[i for i in range(len(b)) if st.comp_of[i % st.bpm] == c], 0]
                diffs |= set(np.diff(dcs).tolist())
            assert {2047, -2047} <= diffs
            print("E %s: before the range limit %d .. %d" % (case.name, lo, hi))


def test_f_saturation_and_colour():
    for case in F.family_f():
        check(case)
        in_window(case)
        st = case.stream
        if getattr(case, "cube", False) or getattr(case, "steps", False):
            pl = R.planes(st, case.sequential[0])
            h = st.h
            y = pl[0][:h.height, :h.width].astype(np.int64)
            if h.mode == "420":
                cb, cr = (R.upsample_h2v2(p, h.height, h.width).astype(np.int64) - 128 for p in pl[1:])
                step = max(int(np.abs(np.diff(p[:h.height // 2, :h.width // 2].astype(np.int64), axis=1)).max()) for p in pl[1:])
                assert step == 255, step                                               # neighbouring chroma samples 0 and 255
            else:
                cb, cr = (p[:h.height, :h.width].astype(np.int64) - 128 for p in pl[1:])
                seen = {(int(a), int(b), int(c)) for a, b, c in zip(y[::8, ::8].ravel(), cb[::8, ::8].ravel() + 128, cr[::8, ::8].ravel() + 128)}
                assert seen == {(a, b, c) for a in F.CUBE for b in F.CUBE for c in F.CUBE}
            rgb = (y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), y + ((116130 * cb + 32768) >> 16))
            for v in rgb:                                                              # each of R, G, B is clamped at both ends
                assert v.min() < 0 and v.max() > 255
            print("F %s: R, G, B before the clamp %s" % (case.name, [(int(v.min()), int(v.max())) for v in rgb]))
    assert {c.stream.h.qt[0, 0] for c in F.family_f() if c.written is None} >= {255}   # quality 1: the coarsest table


def test_g_relaxation_worst_case():
    worst, easy, wide = F.family_g()
    rounds = check(worst)
    in_window(worst)
    nsub = worst.stream.h.nsub
    assert R.DEFAULT_MAX_ROUNDS < rounds <= nsub <= 250, (rounds, nsub)
    assert R.relax(worst.stream, max_rounds=R.DEFAULT_MAX_ROUNDS)[2] is False          # NOT_CONVERGED at the default cap
    assert check(easy) == 1
    check(wide)
    h = wide.stream.h
    sub0 = h.seg_sub0.tolist()
    assert h.nsub > 256 and h.restart_interval > 0
    assert any(a <= 255 and b >= 257 for a, b in zip(sub0[:-1], sub0[1:]))             # one segment lies across subsequence 256
    assert any(a < 256 for a in sub0[1:-1]) and any(a > 256 for a in sub0[1:-1])
    print("G: %d rounds for %d subsequences of periodic content (default cap %d)" % (rounds, nsub, R.DEFAULT_MAX_ROUNDS))


def test_rounds_never_exceed_the_subsequences_of_the_longest_segment():
    largest = 0
    for name, cases in F.cpu_families().items():
        for case in cases:
            rounds = case.relaxed[1]
            assert rounds <= max(seg.m for seg in case.stream.segs), case.name
            largest = max(largest, rounds)
    print("largest number of rounds over every family: %d" % largest)
