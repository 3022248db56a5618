"""The events.csv grammar of ops.parse_events_csv (csrc/events_csv.hip), restated in plain Python / NumPy.

The oracle is event_render.read_events_csv: pandas.read_csv(header=None, comment='#', sep=',' or r'\\s+', names=4 columns)
followed by .values.astype(np.int64).  The device accepts a subset of what that reader accepts, chosen so that on the subset the
result is a function of each line alone (plus one flag per column), and answers "unsupported" everywhere else:

  lines     every '\\n' and every '\\r' ends a line ('\\r\\n' is then a line end followed by an empty line); the text after the
            last one is a line too.  A line is cut at its first '#'.
  skipped   a line that is empty or holds only spaces / tabs (before the cut), and a line whose first byte is '#'.
            Spaces / tabs followed by '#' is NOT a skipped line for the reader in comma mode (it becomes a row with one blank
            field): unsupported in both modes.
  lone '\\r' the reader's tokenizer mishandles two things after a '\\r' that is not followed by '\\n', both unsupported here:
            comma mode, a row that begins with a space / tab (the tokenizer backs up to the previous '\\n' and reads the text
            before the '\\r' again); whitespace mode, a line of only spaces / tabs (it becomes a row of NaN).
  row       exactly four fields; comma mode: separated by ',', spaces / tabs around a field ignored; whitespace mode:
            separated by runs of spaces / tabs, leading and trailing runs ignored.
  field     [+-]? digits [ '.' digits ]  or  [+-]? '.' digits, at least one digit.  Its value is the integer part with the
            sign (truncation toward zero; '-0.9' is 0).
  column    a column in which any field has a '.' is read as float64 by the reader (its 17-digit window counts every digit
            character as written, leading zeros included): accepted only when every field of that column has at most 15 digit
            characters -- then the float64 is the correctly rounded decimal, nearer to it than the decimal is to an integer
            (10^-(15-k) against an ulp of at most 2.3e-16 * 10^k for a k-digit integer part), so truncation gives the integer
            part exactly, and every integer of the column is below 10^15 < 2^53 and survives the round trip.
  ranges    the integer part must fit int64; the x and y columns int32; the polarity column int8 (the device's output types).
  length    a line whose part before any '#' has 65 536 bytes or more is unsupported (one device thread walks a line).
  otherwise exponents, quotes, hex, nan / inf, an empty field, fewer or more than four fields, any other byte: unsupported.

parse(data, ...) returns (t int64, x int32, y int32, p int8) or the string UNSUPPORTED."""
import re

import numpy as np

UNSUPPORTED = "unsupported"
MAX_LINE = 65536

_NUM = rb"([+-]?)(?:([0-9]+)(\.[0-9]*)?|(\.[0-9]+))"
_COMMA = re.compile(rb"[ \t]*" + rb"[ \t]*,[ \t]*".join([_NUM] * 4) + rb"[ \t]*")
_WHITE = re.compile(rb"[ \t]*" + rb"[ \t]+".join([_NUM] * 4) + rb"[ \t]*")
_BLANK = re.compile(rb"[ \t]*")
_LINE = re.compile(rb"([^\r\n]*)(\r\n|\r|\n|$)")
_LIMIT = (2 ** 63, 2 ** 31, 2 ** 31, 2 ** 7)


def parse(data, delim_whitespace=False, swap_xy=False, microseconds_timestamp=False, milliseconds_timestamp=False):
    data = bytes(data)
    pat = _WHITE if delim_whitespace else _COMMA
    cols = ([], [], [], [])
    has_dot = [False] * 4
    over15 = [False] * 4
    order = (0, 2, 1, 3) if swap_xy else (0, 1, 2, 3)        # file column -> output column
    after_cr = False                                         # the previous line ended in a '\r' without '\n'
    for line, end in _LINE.findall(data):
        lone_cr, after_cr = after_cr, end == b"\r"
        cut = line.find(b"#")
        if cut == 0:
            continue
        if cut > 0:
            line = line[:cut]
        if len(line) >= MAX_LINE:
            return UNSUPPORTED                               # one device thread walks a line: its walk is bounded
        if _BLANK.fullmatch(line):
            if cut > 0:
                return UNSUPPORTED                           # blanks, then a comment
            if line and lone_cr and delim_whitespace:
                return UNSUPPORTED                           # the reader makes an empty row of it
            continue
        if lone_cr and not delim_whitespace and line[:1] in (b" ", b"\t"):
            return UNSUPPORTED                               # the reader backs up over the '\r' and reads the text before it again
        m = pat.fullmatch(line)
        if m is None:
            return UNSUPPORTED
        g = m.groups()
        for c in range(4):
            sign, ip, frac, bare = g[4 * c: 4 * c + 4]
            ip = ip or b""
            digits = len(ip) + (len(frac) - 1 if frac else 0) + (len(bare) - 1 if bare else 0)
            if frac is not None or bare is not None:
                has_dot[c] = True
            if digits > 15:
                over15[c] = True
            v = int(ip.lstrip(b"0") or b"0")                  # stripped first: int() refuses very long digit strings
            if sign == b"-":
                v = -v
            oc = order[c]
            if not -_LIMIT[oc] <= v < _LIMIT[oc]:
                return UNSUPPORTED
            cols[oc].append(v)
    if any(d and o for d, o in zip(has_dot, over15)):
        return UNSUPPORTED
    t = np.asarray(cols[0], dtype=np.int64)
    if microseconds_timestamp:
        t = (t.astype(np.float64) / 1000000.0).astype(np.int64)
    elif milliseconds_timestamp:
        t = (t.astype(np.float64) / 1000.0).astype(np.int64)
    return (t, np.asarray(cols[1], dtype=np.int32), np.asarray(cols[2], dtype=np.int32), np.asarray(cols[3], dtype=np.int8))


# ------------------------------------------------------------------------------------------------ the issue's table
ACCEPTED = [        # (name, bytes, delim_whitespace)
    ("lf", b"1,2,3,1\n4,5,6,0\n", False),
    ("crlf", b"1,2,3,1\r\n4,5,6,0\r\n", False),
    ("cr", b"1,2,3,1\r4,5,6,0\r", False),
    ("no_final_line_end", b"1,2,3,1\n4,5,6,0", False),
    ("blank_lines", b"\n1,2,3,1\n\n\n4,5,6,0\n\n", False),
    ("whitespace_only_lines", b"1,2,3,1\n   \n\t\n4,5,6,0\n \t \n", False),
    ("comment_lines", b"# head\n1,2,3,1\n# mid , 1\n4,5,6,0\n#end", False),
    ("trailing_comments", b"1,2,3,1 # c\n4,5,6,0#d\n", False),
    ("padding_comma", b" 1, 2 ,\t3 , 1\n4 ,5,\t6\t, 0 \n", False),
    ("signs_and_zeros", b"+1,-4,001,1\n-0,+0,000,-1\n", False),
    ("whitespace_runs", b"  1 \t 2\t\t3   1  \n4 5 6 0\n\t7\t8\t9\t1\t\n", True),
    ("whitespace_comments", b"# v2e header\n#another\n1.5 2 3 1\n4.25 5 6 0 # c\n7.0 8 9 1#d\n", True),
    ("whitespace_crlf_cr", b"1 2 3 1\r\n4 5 6 0\r7 8 9 1", True),
    ("decimals", b"1.9,2,3,1\n-4.9,5,6,0\n.5,1,1,1\n1.,2,2,0\n0.001234,3,3,1\n", False),
    ("decimal_other_columns", b"10,2.7,3.2,1.0\n20,-0.9,6.,0.4\n", False),
    ("fifteen_digits", b"123456789012345,1,2,1\n12345678901234.5,3,4,0\n", False),
    ("big_integers_no_decimal", b"9007199254740993,1,2,1\n-9223372036854775808,3,4,0\n9223372036854775807,5,6,1\n", False),
    ("int32_edges", b"1,2147483647,-2147483648,1\n2,-2147483648,2147483647,0\n", False),
    ("longest_line", b"0" * (MAX_LINE - 8) + b"7,1,2,1\n4,5,6,0\n" + b" " * (MAX_LINE - 1) + b"\n", False),
    ("long_comment", b"1,2,3,1 #" + b"c" * (2 * MAX_LINE) + b"\n#" + b" " * MAX_LINE + b"\n4,5,6,0\n", False),
    ("empty", b"", False),
    ("comments_only", b"# a\n#b\n\n", False),
    ("blank_only", b"\n\n \n", False),
    ("empty_whitespace_mode", b"", True),
]

REJECTED = [
    ("big_integer_in_decimal_column", b"9007199254740993,1,2,1\n1.5,3,4,0\n", False),
    ("seventeen_digits", b"12345678901.999999,1,2,1\n", False),
    ("exponent", b"1e3,1,2,1\n", False),
    ("exponent_upper", b"1,1E2,2,1\n", False),
    ("quotes", b'"1",1,2,1\n', False),
    ("hex", b"0x10,1,2,1\n", False),
    ("nan", b"nan,1,2,1\n", False),
    ("inf", b"1,inf,2,1\n", False),
    ("three_fields", b"1,2,3\n", False),
    ("three_fields_whitespace", b"1 2 3\n", True),
    ("empty_field", b"1,,3,1\n", False),
    ("five_fields", b"1,2,3,1,9\n", False),
    ("trailing_comma", b"1,2,3,1,\n", False),
    ("five_fields_whitespace", b"1 2 3 1 9\n", True),
    ("beyond_int64", b"9223372036854775808,1,2,1\n", False),
    ("x_beyond_int32", b"1,2147483648,2,1\n", False),
    ("y_beyond_int32", b"1,2,-2147483649,1\n", False),
    ("other_byte", b"1,2,3,1\n4;5;6;0\n", False),
    ("letters", b"t,x,y,p\n1,2,3,1\n", False),
    ("comma_file_in_whitespace_mode", b"1,2,3,1\n", True),
    ("whitespace_file_in_comma_mode", b"1 2 3 1\n", False),
    ("lone_sign", b"-,2,3,1\n", False),
    ("lone_dot", b".,2,3,1\n", False),
    ("two_dots", b"1.2.3,2,3,1\n", False),
    ("inner_space", b"1 0,2,3,1\n", False),
    ("form_feed", b"1,2,3,1\x0c\n", False),
    ("nul", b"1,2,3,1\x00\n", False),
    ("line_too_long", b"0" * (MAX_LINE - 7) + b"7,1,2,1\n4,5,6,0\n", False),
    ("blank_line_too_long", b"1,2,3,1\n" + b" " * MAX_LINE + b"\n4,5,6,0\n", False),
    ("blank_run_too_long", b"1 2 3" + b" " * MAX_LINE + b"1\n", True),
    ("blanks_then_comment", b"1,2,3,1\n  # c\n", False),
]


# ------------------------------------------------------------------------------------------------ seeded corpora
def _line_end(rng):
    return (b"\n", b"\n", b"\n", b"\r\n", b"\r")[int(rng.integers(0, 5))]


def _pad(rng):
    return (b"", b"", b"", b" ", b"\t", b"  ", b" \t")[int(rng.integers(0, 7))]


def _emit(out, line, rng):
    """Append a line with a random line end, keeping clear of the two lone-'\\r' cases the grammar excludes."""
    if out and out[-1].endswith(b"\r"):
        line = line.lstrip(b" \t")
    out.append(line + _line_end(rng))


def _noise(rng, out):
    r = int(rng.integers(0, 40))
    if r == 0:
        _emit(out, b"", rng)
    elif r == 1:
        _emit(out, b"# comment %d, with, commas 1.5e3 \"q\"" % int(rng.integers(0, 1000)), rng)
    elif r == 2:
        _emit(out, _pad(rng), rng)


def corpus_comma(seed, n_lines, hw=(480, 640), padding=True, final_line_end=True):
    """aedat_to_csv.py style: 't,x,y,p' integers, time-sorted; with mixed line ends, blank / comment lines, padding around
    fields, trailing comments and signs when `padding`."""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.integers(0, 40, n_lines)).astype(np.int64) + int(rng.integers(0, 10 ** 9))
    x = rng.integers(0, hw[1], n_lines); y = rng.integers(0, hw[0], n_lines); p = rng.integers(0, 2, n_lines)
    out = []
    for i in range(n_lines):
        if not padding:
            out.append(b"%d,%d,%d,%d\n" % (t[i], x[i], y[i], p[i]))
            continue
        _noise(rng, out)
        f = [b"%d" % t[i], b"%d" % x[i], b"%d" % y[i], b"%d" % p[i]]
        r = int(rng.integers(0, 30))
        if r == 0:
            f[1] = b"+" + f[1]
        elif r == 1:
            f[2] = b"00" + f[2]
        elif r == 2:
            f[3] = b"-" + f[3]
        line = b",".join(_pad(rng) + v + _pad(rng) for v in f)
        if int(rng.integers(0, 25)) == 0:
            line += (b" # c", b"#d")[int(rng.integers(0, 2))]
        _emit(out, line, rng)
    data = b"".join(out)
    if not final_line_end:
        data = data.rstrip(b"\r\n")
    return data


def corpus_white(seed, n_lines, hw=(480, 640), padding=True, final_line_end=True):
    """v2e text style: '%f %d %d %d' (seconds with six decimals), whitespace separated, '#' header lines; written t, y, x, p
    when read with swap_xy."""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.integers(0, 40, n_lines)).astype(np.int64) + int(rng.integers(0, 10 ** 7))
    x = rng.integers(0, hw[1], n_lines); y = rng.integers(0, hw[0], n_lines); p = rng.integers(0, 2, n_lines) * 2 - 1
    out = [b"# v2e text events\n", b"# timestamp(float s) x y polarity(-1 / +1)\n"]
    for i in range(n_lines):
        stamp = b"%d.%06d" % (t[i] // 1000000, t[i] % 1000000)
        if not padding:
            out.append(b"%s %d %d %d\n" % (stamp, x[i], y[i], p[i]))
            continue
        _noise(rng, out)
        seps = [(b" ", b" ", b"\t", b"  ", b" \t ")[int(rng.integers(0, 5))] for _ in range(3)]
        line = _pad(rng) + stamp + seps[0] + b"%d" % x[i] + seps[1] + b"%d" % y[i] + seps[2] + b"%d" % p[i] + _pad(rng)
        if int(rng.integers(0, 25)) == 0:
            line += (b" # c", b"#d")[int(rng.integers(0, 2))]
        _emit(out, line, rng)
    data = b"".join(out)
    if not final_line_end:
        data = data.rstrip(b"\r\n \t")
    return data
