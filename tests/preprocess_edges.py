"""Cases for the text pre-pass's edge suite (tests/test_gpu_preprocess_edges.py runs them on the GPU against oracle/gz_oracle.py,
tests/test_preprocess_edges_inputs.py proves on the CPU that every case sits where it says).  No GPU, no torch; nothing here computes
an expected output.

T = 64 is the trip of pp_filter (csrc/gz_preproc.inc): one wave walks a document 64 bytes at a time and carries what a regular
expression would hold as matcher state in wave-uniform flags from trip to trip.  A case puts one ITEM -- a tag, a URL, a whitespace
run, a base letter and its mark -- where such a flag has to cross a trip edge.

Swept cases: document = prefix + item + suffix, for every
  item    of ITEMS[filter]
  edge    E = T and E = 2 T
  offset  o of the item's first byte in offsets(len(item), E) = [E - len - 1, E + 1]: the item ends one byte before the edge, ends at
          it, straddles it at every byte split, begins at it, begins one byte after it.  Consecutive offsets give the fused kernel's
          dword reads all four alignments p & 3.  An item too long for that inside 3 T bytes has its offsets clipped to
          [0, 3 T - len - len(" tail")]; it then straddles both edges.
  prefix  of PREFIXES[filter], padded to o bytes with the neutral letter x, where o is long enough to hold it:
            plain    letters
            space    letters ending in one ASCII space
            ws       whitespace only (U+3000 and spaces): nothing is kept before the item
            carried  the structure that opens the filter's state at byte 0, then nothing of interest up to the item:
                       html  '<' and letters           url  'http://a' and non-whitespace
                       emoji ' ' and deleted characters only (ws0); 'x ' and deleted characters only (seen)
  suffix  nothing ("end": the last trip is not full unless the item ends at the edge) and " tail" (a kept character follows)
No swept document is longer than 3 T bytes.  cases(filter) adds to them the fixed documents whose layout is their point (a structure at
byte 0, runs that fill whole trips, the 24 x 5 composition table with every base at a trip's last lane).

`fires` of a case: True -- the item's own filter must change the document; False -- it must leave it alone (only stated with the
plain prefix: a lone '>', http + whitespace, x + mark, the kept class borders, U+24C1); None -- depends on the neighbours.

SWEEPS lists the filter chains and whose cases each runs over; probes() are the documents for the fused kernel's skip tests
(ppf_has_byte, ppf_has_http); pack_batches() the batches for gz_pp_pack4_kernel and gz_launch_pp_tail; long_document() the one document
of the mixed batches that the filter-by-filter chain takes.
"""
import collections

import numpy as np

T = 64
EDGES = (T, 2 * T)
MAX_DOC = 3 * T
FILL = b"x"                       # neutral: no base letter of convert_unicode, no punctuation, no whitespace
TAIL = b" tail"
SUFFIXES = (("end", b""), ("tail", TAIL))
KINDS = ("ends_before", "ends_at", "straddles", "begins_at", "begins_after")
FILTERS = ("html", "url", "punct", "emoji", "unicode")

Case = collections.namedtuple("Case", "filt name doc first last edge kind fires item prefix suffix")
Item = collections.namedtuple("Item", "name data fires suffixes")


def u(s):
    return s.encode("utf-8", "surrogatepass")


def text_of(doc: bytes) -> str:
    return doc.decode("utf-8", "surrogatepass")


def cp(*points):
    return u("".join(chr(p) for p in points))


HEART, GRIN = cp(0x2764), cp(0x1F600)                     # deleted by remove_emoji: 3 and 4 bytes
NBSP, IDEO = cp(0xA0), cp(0x3000)                         # whitespace of 2 and 3 bytes
ACUTE, GRAVE, DOT, CIRC = cp(0x301), cp(0x300), cp(0x323), cp(0x302)      # CIRC: a 0xCC-led mark that is no tone mark
E_ACUTE, E_DOT = cp(0xE9), cp(0x1EC7)                     # kept characters of 2 and 3 bytes
ACIRC, UHORN = cp(0xE2), cp(0x1B0)                        # base letters of 2 bytes
PUNCT = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"
BORDERS = (0x20, 0x30, 0x39, 0x41, 0x5A, 0x61, 0x7A, 0x7F)     # the neighbours of the punctuation classes: kept
# a a-circumflex a-breve e e-circumflex i o o-circumflex o-horn u u-horn y, and their capitals; grave acute hook tilde dot-below
BASES = "".join(chr(p) for p in (0x61, 0xE2, 0x103, 0x65, 0xEA, 0x69, 0x6F, 0xF4, 0x1A1, 0x75, 0x1B0, 0x79,
                                 0x41, 0xC2, 0x102, 0x45, 0xCA, 0x49, 0x4F, 0xD4, 0x1A0, 0x55, 0x1AF, 0x59))
MARKS = "".join(chr(p) for p in (0x300, 0x301, 0x309, 0x303, 0x323))


def it(name, data, fires, suffixes=("end", "tail")):
    return Item(name, data if isinstance(data, bytes) else u(data), fires, tuple(suffixes))


ITEMS = {
    "html": [
        it("b_tag", "<b>", True), it("empty_tag", "<>", True), it("tag72", "<" + "q" * 70 + ">", True),
        it("lone_gt", "a>b", False), it("lt_in_tag", "<a<b>", True), it("unclosed_last", "<a>x<b", True),
        it("unclosed_at_end", "<a", False, ("end",)), it("unclosed_then_text", "<a", False, ("tail",)),
        it("gt_T_later", "<" + "q" * (T - 1) + ">", True), it("gt_2T_later", "<" + "q" * (2 * T - 1) + ">", True),
        it("two_tags", "<a><b>", True), it("newline_in_tag", "<a\nb>", True),
        it("closed_then_open", "<a><", True), it("nested", "<<>>", True), it("gt_lt", "><", False), it("tag_gt", "<a>>", True),
    ],
    "url": [
        it("http_end", b"http", False, ("end",)),
        it("http_sp", b"http ", False), it("http_nbsp", b"http" + NBSP, False), it("http_ideo", b"http" + IDEO, False),
        it("http_c1", b"httpy", True), it("http_c2", b"http" + E_ACUTE, True), it("http_c3", b"http" + E_DOT, True),
        it("http_c4", b"http" + GRIN, True),
        it("mid_run", b"xhttpy", True), it("httphttp", b"httphttp://a", True), it("http_http", b"http http://a", True),
        it("url_sp", b"http://ab K", True), it("url_nbsp", b"http://ab" + NBSP + b"K", True), it("url_ideo", b"http://ab" + IDEO + b"K", True),
        it("longurl_sp", b"http://" + b"u" * 66 + b" K", True), it("longurl_nbsp", b"http://" + b"u" * 66 + NBSP + b"K", True),
        it("longurl_ideo", b"http://" + b"u" * 66 + IDEO + b"K", True),
        it("https", b"https", True), it("http_nl", b"http\n", False), it("upper", b"HTTP://a", False), it("htthttp", b"htthttp://a", True),
        it("url_tab_url", b"http://a\thttp://b", True),
    ],
    "punct": [it("punct_%02X" % ord(c), c, True) for c in PUNCT] + [it("border_%02X" % b, bytes([b]), False) for b in BORDERS],
    "emoji": [
        it("del3", HEART, True), it("del4", GRIN, True), it("zwj", cp(0x200D), True), it("watch", cp(0x231A), True),
        it("kept_24C1", cp(0x24C1), False), it("del_24C2", cp(0x24C2), True), it("kept3", E_DOT, False), it("kept2", E_ACUTE, False),
        it("vs16", cp(0x2764, 0xFE0F), True), it("lone_surrogate", cp(0xD83D), True),
        it("ws1", b" ", None), it("ws2", NBSP, True), it("ws3", IDEO, True), it("tab", b"\t", True), it("nel", cp(0x85), True),
        it("ogham", cp(0x1680), True), it("em_space", cp(0x2003), True),
        it("ws_del_ws", b" " + HEART + b" ", True), it("del_ws_del", HEART + b" " + GRIN, True, ("end",)),
        it("del_ws_del_text", HEART + b" " + GRIN, True, ("tail",)),
        it("kept_del_kept", b"a" + HEART + b"b", True), it("kept_ws_del_kept", b"a " + HEART + b"b", True),
        it("kept_del_ws_kept", b"a" + HEART + IDEO + b"b", True),
        it("wsrun64", b"a" + b" " * T + b"b", True), it("wsrun65", b"a" + b" " * (T + 1) + b"b", True),
        it("wsrun64_ideo", b"a" + IDEO * 21 + b" b", True),
        it("delrun_pend", b"a " + HEART * 22 + b"b", True), it("delrun_nopend", b"a" + HEART * 22 + b"b", True),
        it("delrun4_pend", b"a " + GRIN * 16 + b"b", True),
        it("ws_punct_ws", b" ! ", None), it("nbsp_punct_ideo", NBSP + b"!" + IDEO, True),
    ],
    "unicode": [
        it("a_acute", b"a" + ACUTE, True), it("acirc_acute", ACIRC + ACUTE, True), it("uhorn_dot", UHORN + DOT, True),
        it("x_acute", b"x" + ACUTE, False), it("a_acute_acute", b"a" + ACUTE + ACUTE, True), it("aa_acute", b"aa" + ACUTE, True),
        it("a_circumflex_mark", b"a" + CIRC, False), it("a_macron_mark", b"a" + cp(0x304), False), it("a_cd_mark", b"a" + cp(0x340), False),
        it("two_pairs", b"e" + ACUTE + b"o" + GRAVE, True), it("mark_a_acute", ACUTE + b"a" + ACUTE, True),
        it("three_byte_then_mark", cp(0x1EA1) + ACUTE, False), it("upper_pair", b"Y" + cp(0x309), True),
        it("composed_then_mark", cp(0xE1) + ACUTE, False), it("acirc_alone", ACIRC, False), it("mark_alone", ACUTE, None),
    ],
}


# ---------------------------------------------------------------------------------------------------------------------------------
# prefixes: o -> bytes of length o, or None where o cannot hold it
def _dels(n):
    """n bytes of deleted characters (3 a + 4 b); None for 1, 2 and 5"""
    b = n % 3
    a = (n - 4 * b) // 3
    return HEART * a + GRIN * b if a >= 0 else None


def p_plain(o):
    return FILL * o


def p_space(o):
    return FILL * (o - 1) + b" " if o >= 1 else None


def p_ws(o):
    return IDEO * (o // 3) + b" " * (o % 3) if o >= 1 else None


def p_lt(o):
    return b"<" + FILL * (o - 1) if o >= 1 else None


def p_url(o):
    return b"http://a" + b"u" * (o - 8) if o >= 8 else None


def _ws_then_dels(head, o):
    for r in range(4):                                          # 1, 2 and 5 bytes: more spaces instead
        n = o - len(head) - r
        if n >= 0 and _dels(n) is not None:
            return head + b" " * r + _dels(n)
    return None


def p_ws0(o):
    return _ws_then_dels(b" ", o) if o >= 1 else None


def p_seen(o):
    return _ws_then_dels(b"x ", o) if o >= 2 else None


NEUTRAL = [("plain", p_plain), ("space", p_space), ("ws", p_ws)]
PREFIXES = {
    "html": NEUTRAL + [("carried", p_lt)],
    "url": NEUTRAL + [("carried", p_url)],
    "punct": NEUTRAL,
    "emoji": NEUTRAL + [("carried_ws0", p_ws0), ("carried_seen", p_seen)],
    "unicode": NEUTRAL,
}


def offsets(n, edge):
    return range(max(0, edge - n - 1), min(edge + 1, MAX_DOC - n - len(TAIL)) + 1)


def kind_of(first, last, edge):
    if last == edge - 2:
        return "ends_before"
    if last == edge - 1:
        return "ends_at"
    if first == edge:
        return "begins_at"
    if first == edge + 1:
        return "begins_after"
    assert first <= edge - 1 < last, (first, last, edge)
    return "straddles"


def _swept(filt):
    out = []
    for item in ITEMS[filt]:
        n = len(item.data)
        for edge in EDGES:
            for o in offsets(n, edge):
                for pname, pfn in PREFIXES[filt]:
                    pre = pfn(o)
                    if pre is None:
                        continue
                    assert len(pre) == o, (filt, pname, o)
                    for sname, suf in SUFFIXES:
                        if sname not in item.suffixes:
                            continue
                        fires = True if item.fires is True else False if (item.fires is False and pname == "plain") else None
                        name = "%s/%s/E%d/o%d/%s/%s" % (filt, item.name, edge, o, pname, sname)
                        out.append(Case(filt, name, pre + item.data + suf, o, o + n - 1, edge, kind_of(o, o + n - 1, edge), fires,
                                        item.name, pname, sname))
    return out


def _fixed_case(filt, name, pre, data, suf, fires):
    pre, data, suf = (x if isinstance(x, bytes) else u(x) for x in (pre, data, suf))
    return Case(filt, "%s/fixed/%s" % (filt, name), pre + data + suf, len(pre), len(pre) + len(data) - 1, None, "fixed", fires, name, "fixed", "fixed")


def _fixed(filt):
    f = lambda *a: _fixed_case(filt, *a)
    out = []
    if filt == "html":
        for k in (T - 3, T - 2, T - 1, T, T + 1):              # a tag opened at byte 0 that closes around the edge / never closes
            out.append(f("tag_from_0_len%d" % (k + 1), b"", b"<" + b"q" * (k - 1) + b">", b"z", True))
            out.append(f("open_from_0_len%d" % k, b"", b"<" + b"q" * (k - 1), b"", False))
        out.append(f("only_lt", b"", b"<", b"", False))
        out.append(f("lt_run", b"", b"<" * (T + 2), b">", True))
        out.append(f("gt_run_then_lt_run", b"a" * T, b">" + b"<" * T, b"", False))
    elif filt == "url":
        for k in (T - 10, T - 9, T - 8, T - 7):                # a URL at byte 0 ended by whitespace around the edge
            for w, ws in (("sp", b" "), ("nbsp", NBSP), ("ideo", IDEO)):
                out.append(f("url_at_0_%s_%d" % (w, k), b"", b"http://a" + b"u" * k + ws + b"K", b"", True))
        out.append(f("url_at_0", b"", b"http://a b", b"", True))
        out.append(f("http_only", b"", b"http", b"", False))
        out.append(f("url_to_the_end", b"", b"http" + b"u" * (2 * T), b"", True))
    elif filt == "punct":
        out.append(f("all_punct", b"", PUNCT.encode() * 4, b"", True))
        out.append(f("all_borders", b"", bytes(BORDERS) * 9, b"", False))
    elif filt == "emoji":
        for k in (T - 8, T - 7, T - 6, T - 5):                 # deleted + whitespace + deleted at the document's start
            out.append(f("del_ws_del_at_0_%d" % k, b"", HEART + b" " + GRIN, b"y" * k + b" z", True))
        out.append(f("only_ws", b"", b" " * (T + 1), b"", True))
        out.append(f("only_del", b"", HEART * 22, b"", True))
        out.append(f("only_ws_and_del", b"", (b" " + GRIN) * 13, b"", True))
        out.append(f("ws_run_at_0_T", b"", b" " * T, b"y", True))
        out.append(f("ws_run_at_0_T1", b"", b" " * (T + 1), b"y", True))
        out.append(f("trip_of_ws_then_trip_of_del", b"a", b" " * (T - 1) + GRIN * 16, b"b", True))
        out.append(f("trip_of_del_then_trip_of_ws", b"a", HEART * 21 + b" " * T, b"b", True))
    else:
        # the 24 x 5 table once: the base's last byte at a trip's last lane, the mark in the next trip
        k = 0
        for b in BASES:
            for m in MARKS:
                edge = EDGES[k % 2]
                k += 1
                out.append(f("table_%04X_%04X" % (ord(b), ord(m)), FILL * (edge - len(u(b))), b + m, b"" if k % 3 else TAIL, True))
        out.append(f("mark_at_0", b"", ACUTE, b"a" * T, False))
        out.append(f("mark_at_0_then_pair", b"", ACUTE, b"a" + ACUTE, True))
        out.append(f("pair_at_0", b"", b"a" + ACUTE, b"", True))
        out.append(f("pairs_only", b"", (b"a" + ACUTE) * 40, b"", True))
        out.append(f("two_byte_pairs_only", b"", (ACIRC + ACUTE) * 33, b"", True))
    return out


_CASES = {}


def cases(filt):
    """The swept and the fixed cases built for one filter."""
    if filt not in _CASES:
        _CASES[filt] = _swept(filt) + _fixed(filt)
    return _CASES[filt]


ALL5 = ("html", "url", "unicode", "punct", "emoji")
# (filter chain, the filters whose cases it runs over)
SWEEPS = [((f,), (f,)) for f in FILTERS] + [
    (("punct", "emoji"), ("punct", "emoji")), (("emoji", "punct"), ("punct", "emoji")),
    (ALL5, FILTERS), (("url", "html"), FILTERS),
    (("unicode", "unicode"), ("unicode",)),
    (("html", "unicode", "emoji"), ("html", "unicode", "emoji")),          # a chain of three: with 1, 2 and 5 both parities of the ping-pong
]


def chain_id(chain):
    return "+".join(chain)


def sweep_cases(over):
    return [c for f in over for c in cases(f)]


def pack(docs):
    """documents (bytes) -> packed uint8 text (with readable bytes behind it), int64 offsets"""
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    raw = b"".join(docs)
    return np.frombuffer(raw + b"\0" * 16, np.uint8)[:len(raw)], off


# ---------------------------------------------------------------------------------------------------------------------------------
Probe = collections.namedtuple("Probe", "name doc filt fires")


def probes():
    """Documents for which the skip tests must answer yes (`fires`: and the filter then changes them), and their "no" forms: the same
    documents without the last byte -- without the last character where that byte is a mark's second."""
    out = []
    for i in range(12):                                         # every dword phase, the fifth byte the document's last
        d = b"y" * i + b"httpx"
        out.append(Probe("http_at_%d" % i, d, "url", True))
        out.append(Probe("http_at_%d_cut" % i, d[:-1], "url", False))
    for length in range(1, 13):
        for k, tag in enumerate((b"<", b"<>", b"<a>", b"<ab>"), 1):       # a '<' among the last 1 .. 4 bytes
            if length >= k:
                d = b"y" * (length - k) + tag
                out.append(Probe("lt_last_%d_of_%d" % (k, length), d, "html", k > 1))
                out.append(Probe("lt_last_%d_of_%d_cut" % (k, length), d[:-1], "html", False))
        for k, behind in ((2, b""), (3, b"z"), (4, b"zz")):               # the mark's 0xCC among the last 2 .. 4 bytes, behind a base
            if length >= k + 1:
                d = b"y" * (length - k - 1) + b"a" + ACUTE + behind
                out.append(Probe("mark_last_%d_of_%d" % (k, length), d, "unicode", True))
                cut = d[:-1] if behind else d[:-2]
                out.append(Probe("mark_last_%d_of_%d_cut" % (k, length), cut, "unicode", bool(behind)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
PACK_NDOCS = (1, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025)
PACK_OUT_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257)
PACK_MAX_DOC = 262
_LETTERS = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def _mix(d, i):
    x = (d * 0x9E3779B1 + i * 0x85EBCA6B + 1) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    return x ^ (x >> 12)


def pack_doc(d):
    """document d of a pack batch: PACK_OUT_LENS[d % 14] letters, every one a function of (d, i), and d % 6 '!' behind them"""
    n = PACK_OUT_LENS[d % len(PACK_OUT_LENS)]
    return bytes(_LETTERS[_mix(d, i) % 52] for i in range(n)) + b"!" * (d % 6)


def pack_batches():
    return {n: [pack_doc(d) for d in range(n)] for n in PACK_NDOCS}


# ---------------------------------------------------------------------------------------------------------------------------------
LONG_BYTES = 4097 + T


def long_document():
    """4 097 + 64 bytes of letters with one item of each filter at a trip edge: longer than the fused kernel takes."""
    parts = [(3 * T - 1, b"<b>"), (10 * T - 10, b"http://ab" + IDEO + b"K"), (20 * T - 1, b"!?"), (30 * T - 2, b" " + HEART + b" "),
             (40 * T - 1, b"a" + ACUTE), (50 * T - 2, ACIRC + ACUTE), (60 * T - 1, GRIN), (LONG_BYTES - 2, b"<a")]
    doc = b""
    for at, item in parts:
        assert at >= len(doc)
        doc += b"z" * (at - len(doc)) + item
    assert len(doc) == LONG_BYTES
    return doc
