"""The Zstandard payloads the ZSTD tests share: plans for tests/zstd_stream_writer.py that force each rule of the format at the
smallest size (valid(): name -> (payload, the bytes it stands for)) and damaged payloads (refused(): name -> (payload, status with
verify, status without)).  Built once per process."""
import functools
import struct

import numpy as np

import zstd_stream_writer as Z

CORRUPT, CHECKSUM = 1, 2
TEXT = bytes(range(65, 91)) * 3
# literals whose plain Huffman code is 11 bits deep: frequencies 1, 1, 2, 4, ... 1024
DEEP = bytes(s for s, c in enumerate([1, 1] + [1 << k for k in range(1, 11)]) for _ in range(c))
SEQ = [(4, 7, 5), (0, 1, 4), (3, 2, 6), (2, 3, 3), (0, 3, 4), (1, 1, 7), (0, 2, 3)]       # every repeat code, ll zero and not


def _lits(seqs, extra=5, seed=1):
    n = sum(s[0] for s in seqs) + extra
    return bytes(np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8))


SEQ2 = [(4, 9, 5), (1, 1, 4), (3, 2, 6), (2, 3, 3)]


def _many(n, spread=5):
    return [(1, 4, 3)] + [(1 if i % 3 else 0, 1 + i % 3, 3 + i % spread) for i in range(n - 1)]


@functools.lru_cache(maxsize=None)
def valid():
    c, out = Z.compressed, {}

    def add(name, blocks, **kw):
        out[name] = Z.frame(blocks, **kw)

    add("raw_block", [Z.raw(TEXT)])
    add("rle_block", [Z.rle(0x41, 1000), Z.raw(b"xyz")])
    add("empty", [Z.raw(b"")], single=True)
    add("literals_raw", [c(TEXT)])
    add("literals_raw_format1", [c(TEXT * 2, lit_format=1)])
    add("literals_raw_format3", [c(TEXT, lit_format=3)])
    add("literals_rle", [c(b"z" * 300, lit="rle")])
    add("literals_rle_odd_size", [c(b"z" * 21, lit="rle")])                                 # bit 3 of the header belongs to the size
    add("huffman_one_stream", [c(TEXT * 2, lit="huffman")])
    add("huffman_four_streams", [c(TEXT * 9 + b"AB", lit="huffman", streams=4)])
    add("huffman_four_streams_format3", [c(TEXT * 9, lit="huffman", streams=4, lit_format=3)])
    add("huffman_stream_of_zero", [c(b"ABABAA", lit="huffman", streams=4)])                # 2, 2, 2 and 0 literals
    add("huffman_fse_weights", [c(TEXT * 2, lit="huffman", tree="fse")])
    add("huffman_fse_weights_odd", [c(TEXT[:25] * 3, lit="huffman", tree="fse", streams=4)])
    add("huffman_11_bits", [c(DEEP, lit="huffman", streams=4)])
    add("treeless", [c(TEXT * 2, lit="huffman"), c(TEXT[::-1], lit="treeless"), c(TEXT, lit="treeless", streams=4)])
    add("sequences_predefined", [c(_lits(SEQ), SEQ)])
    add("sequences_rle", [c(b"abcdefgh" + b"q" * 12, [(2, 5, 4)] * 6, ll="rle", of="rle", ml="rle")])
    add("sequences_fse", [c(_lits(SEQ), SEQ, ll="fse", of="fse", ml="fse")])
    add("sequences_fse_logs", [c(_lits(_many(300)), _many(300), ll="fse", of="fse", ml="fse", ll_log=9, of_log=8, ml_log=9)])
    add("sequences_repeat", [c(_lits(SEQ), SEQ, ll="fse", of="fse", ml="fse"), c(_lits(SEQ, seed=2), SEQ, ll="repeat", of="repeat", ml="repeat"),
                             c(_lits(SEQ2, seed=3), SEQ2), c(_lits(SEQ2, seed=4), SEQ2, ll="repeat", of="repeat", ml="repeat")])
    add("sequences_mixed", [c(_lits(SEQ), SEQ, ll="fse"), c(_lits(SEQ), SEQ, ll="repeat", of="fse", ml="predefined"),
                            c(b"abcdefgh" * 3, [(2, 5, 4)] * 6, ll="rle", of="repeat", ml="rle")])
    add("sequences_127", [c(_lits(_many(127)), _many(127))])
    add("sequences_128", [c(_lits(_many(128)), _many(128))])
    add("sequences_0x7eff", [c(_lits(_many(0x7EFF, 1)), _many(0x7EFF, 1))])
    add("sequences_0x7f00", [c(_lits(_many(0x7F00, 1)), _many(0x7F00, 1), lit="huffman", streams=4)])
    add("overlap_offset_1", [c(b"ab", [(2, 4, 40)])])
    add("long_lengths", [c(b"x" * 66000 + b"yz", [(66000, 4, 3)]), c(b"", [(0, 66000 + 3, 65600)])])   # the last LL and ML codes
    add("rep1_minus_1", [c(b"abcdefgh", [(8, 5 + 3, 3), (0, 3, 4)])])                      # offset 5, then 4
    add("window_1k_offset_at_window", [Z.raw(bytes(range(256)) * 4), c(b"", [(0, 1024 + 3, 8)])], window=0)
    # block 1 leaves the repeat offsets 13, 11, 7; block 2 opens with repeat codes that resolve to 7, 13 and 13 again.  A decoder
    # that reset the history at the seam would copy from 8, 1 and 1
    add("repeat_offsets_across_blocks", [c(_lits([], 45, seed=6), [(20, 7 + 3, 4), (3, 11 + 3, 5), (2, 13 + 3, 6)]),
                                         c(b"Q!", [(1, 3, 5), (0, 1, 4), (1, 1, 3)])])
    add("match_into_previous_block", [c(TEXT, [(10, 4, 3)]), c(b"!", [(1, 60 + 3, 30), (0, 1, 5)])])
    for nbytes in (0, 2, 4, 8):
        add("fcs_%d" % nbytes, [c(TEXT * 4, [(30, 26 + 3, 20)])], fcs_bytes=nbytes)
    add("fcs_1_single_segment", [c(TEXT, [(30, 26 + 3, 20)])], single=True)
    add("fcs_2_single_segment", [c(TEXT * 4, lit="huffman")], single=True)
    add("unused_bit", [Z.raw(TEXT)], descriptor_or=0x10)
    add("dictionary_id_zero", [Z.raw(TEXT)], did=b"\0\0")
    add("checksum", [c(_lits(SEQ), SEQ), Z.rle(7, 99)], checksum=True)
    two = [Z.frame([c(TEXT, [(30, 26 + 3, 20)])], checksum=True), Z.frame([Z.raw(b"second"), c(b"ab", [(2, 4, 9)])])]
    out["two_frames"] = (two[0][0] + two[1][0], two[0][1] + two[1][1])
    out["skippable_first"] = (Z.skippable() + two[0][0] + Z.skippable(b"", 15), two[0][1])
    return out


def _poke(data, at, value):
    b = bytearray(data)
    b[at] = value
    return bytes(b)


@functools.lru_cache(maxsize=None)
def refused():
    c, out = Z.compressed, {}
    both = lambda payload: (payload, CORRUPT, CORRUPT)                                      # noqa: E731
    good = Z.frame([c(Z_TEXT, SEQ, lit="huffman", ll="fse", of="fse", ml="fse")])[0]
    out["wrong_magic"] = both(Z.frame([Z.raw(TEXT)], magic=0xFD2FB527)[0])
    out["lz4_magic"] = both(b"\x04\x22\x4d\x18" + good[4:])
    out["empty_payload"] = both(b"")
    out["only_skippable"] = both(Z.skippable())
    out["dictionary_id"] = both(Z.frame([Z.raw(TEXT)], did=b"\x07")[0])
    out["reserved_bit"] = both(Z.frame([Z.raw(TEXT)], descriptor_or=8)[0])
    out["block_type_3"] = both(Z.frame([("bytes", 3, 4, b"abcd")])[0])
    out["block_above_window"] = both(Z.frame([Z.raw(b"a" * 1025)], window=0)[0])
    out["cut_at_block_header"] = both(good[:7])
    out["cut_at_frame_header"] = both(good[:5])
    out["cut_in_raw_block"] = both(Z.frame([Z.raw(TEXT)])[0][:-3])
    out["no_last_block"] = both(Z.frame([Z.raw(TEXT)])[0][:6] + Z.Writer().block(Z.raw(TEXT), False))
    # a Compressed block whose size field says more than the payload holds, cut at each part
    for name, keep in (("literals", 12), ("table", 45), ("bitstream", len(good) - 2)):
        out["overrun_cut_at_" + name] = both(good[:keep])
    # the same cuts INSIDE a block whose header is honest about the shorter size
    for name, cut in (("bitstream", 3), ("tables", 12)):
        out["block_ends_in_" + name] = both(Z.frame([c(Z_TEXT, SEQ, lit="huffman", ll="fse", of="fse", ml="fse", cut=cut)])[0])
    out["treeless_first"] = both(_treeless_first())
    out["repeat_first"] = both(_repeat_first())
    out["repeat_after_literals_only"] = both(_repeat_first(first=[c(TEXT)]))
    out["offset_zero"] = both(Z.frame([c(b"abcd", [(4, 3, 3), (0, 3, 3), (0, 3, 3), (0, 3, 3)], execute=False)])[0])   # rep1 - 1 down to 0
    out["offset_before_frame_start"] = both(Z.frame([Z.raw(b"first frame " * 4)])[0] + Z.frame([c(b"abcd", [(4, 5 + 3, 3)], execute=False)])[0])
    out["offset_beyond_window"] = both(Z.frame([Z.raw(bytes(1200)), c(b"", [(0, 1025 + 3, 8)], execute=False)], window=0)[0])
    out["fcs_too_small"] = both(Z.frame([c(TEXT * 4)], fcs_bytes=4, fcs=311)[0])
    out["fcs_too_large"] = both(Z.frame([c(TEXT * 4)], fcs_bytes=2, fcs=313)[0])
    out["fcs_above_cap"] = both(Z.frame([c(TEXT * 4)], fcs_bytes=8, fcs=1 << 40)[0])
    for kind, limit in (("ll", 9), ("of", 8), ("ml", 9)):
        norm = Z.normalize([c0[0] for c0 in ([Z._code(s[0], Z.LL_CODES) for s in SEQ] if kind == "ll" else
                                             [(s[1].bit_length() - 1,) for s in SEQ] if kind == "of" else
                                             [Z._code(s[2], Z.ML_CODES) for s in SEQ])], limit + 1, 53)
        out["accuracy_above_limit_" + kind] = both(Z.frame([c(_lits(SEQ), SEQ, **{kind: "fse", kind + "_log": limit + 1, kind + "_norm": norm})])[0])
    out["weights_accuracy_above_limit"] = both(Z.frame([c(TEXT * 2, lit="huffman", tree="fse", tree_log=7)])[0])
    out["weights_not_power_of_two"] = both(_bad_weights())
    out["modes_reserved_bits"] = both(Z.frame([c(_lits(SEQ), SEQ, reserved_modes=1)])[0])
    out["literals_run_out"] = both(Z.frame([c(b"abc", [(2, 4, 3), (2, 1, 3)], execute=False)])[0])
    out["bitstream_without_marker"] = both(Z.frame([c(_lits(SEQ), SEQ, tail=b"\x12\x00")])[0])
    out["bitstream_not_consumed"] = both(_spare_bits())
    out["rle_symbol_out_of_range"] = both(Z.frame([c(b"abcdefgh" * 3, [(2, 5, 4)] * 6, ll="rle", ll_symbol=36)])[0])
    out["trailing_garbage"] = both(good + b"\0")
    bad = Z.frame([c(_lits(SEQ), SEQ), Z.rle(7, 99)], checksum=True, bad_checksum=True)[0]
    out["wrong_checksum"] = (bad, CHECKSUM, 0)
    out["cut_in_checksum"] = both(bad[:-2])
    return out


Z_TEXT = TEXT * 2 + _lits(SEQ)


def _treeless_first():
    w = Z.Writer()
    w.weights = Z.huffman_weights(TEXT)
    return w.frame([Z.compressed(TEXT, lit="treeless")])[0]


def _repeat_first(first=()):
    w = Z.Writer()
    w.table("ll", [0], 36, {})
    return w.frame(list(first) + [Z.compressed(_lits(SEQ), SEQ, ll="repeat")])[0]


def _bad_weights():
    # direct weights 1, 1, 1 for 'A', 'B', 'C' and an implied one for 'D': 3 is completed to 4 by ONE weight of 1 -- fine; weights
    # 2, 1, 1, 1 for four symbols sum to 5, whose gap to 8 is 3: no single weight fills it
    tree = bytes([127 + 69]) + bytes(32) + b"\x02\x11\x10"
    w = Z.Writer()
    w.weights = {65: 2, 66: 2}
    return w.frame([Z.compressed(b"ABAB" * 4, lit="huffman", weights={65: 2, 66: 2}, tree_bytes=tree)])[0]


def _spare_bits():
    # a valid sequence bitstream with one more zero bit under the end marker: the decoder is left with a bit it may not ignore
    frame = Z.frame([Z.compressed(_lits(SEQ), SEQ, tail=b"")])[0]
    whole = Z.frame([Z.compressed(_lits(SEQ), SEQ)])[0]
    stream = whole[len(frame):]
    value = int.from_bytes(stream, "little")
    longer = (value << 1).to_bytes(len(stream) + (1 if value.bit_length() % 8 == 0 else 0), "little")
    return Z.frame([Z.compressed(_lits(SEQ), SEQ, tail=longer)])[0]
