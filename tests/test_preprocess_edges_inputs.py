"""Host-only: every case of tests/preprocess_edges.py sits on the edge it is built for, fires (or must not) under the oracle, and the
oracle's filters agree with the regular expressions they restate.  Layouts are recomputed from the documents' bytes, counts from the
products the cases are generated from.  Nothing runs on a GPU."""
import collections
import re
import string

import pytest

import gz_oracle as O
import preprocess_edges as E

T = 64
# shortest offset that holds each prefix (the module's builders return None below it)
PREFIX_MIN = {"plain": 0, "space": 1, "ws": 1, "carried": {"html": 1, "url": 8}, "carried_ws0": 1, "carried_seen": 2}
PREFIX_NAMES = {"html": ["plain", "space", "ws", "carried"], "url": ["plain", "space", "ws", "carried"], "punct": ["plain", "space", "ws"],
                "emoji": ["plain", "space", "ws", "carried_ws0", "carried_seen"], "unicode": ["plain", "space", "ws"]}
# cases per filter and per chain as printed by test_case_counts when this file was written: the list cannot grow unnoticed
MEASURED = {"html": 4277, "url": 6435, "punct": 1922, "emoji": 10791, "unicode": 1409}
FIXED = {"html": 13, "url": 15, "punct": 2, "emoji": 11, "unicode": 125}


def prefix_min(filt, pname):
    m = PREFIX_MIN[pname]
    return m[filt] if isinstance(m, dict) else m


def item_offsets(n, edge):
    """restated: [E - n - 1, E + 1], clipped to what 3 T bytes hold with " tail" behind the item"""
    return [o for o in range(edge - n - 1, edge + 2) if o >= 0 and o + n + 5 <= 3 * T]


@pytest.mark.parametrize("filt", E.FILTERS)
def test_swept_cases_sit_on_their_edges_and_none_is_missing(filt):
    items = {i.name: i for i in E.ITEMS[filt]}
    assert len(items) == len(E.ITEMS[filt])
    assert [p for p, _ in E.PREFIXES[filt]] == PREFIX_NAMES[filt]
    swept = [c for c in E.cases(filt) if c.kind != "fixed"]
    names = collections.Counter(c.name for c in E.cases(filt))
    assert max(names.values()) == 1
    have = collections.Counter()
    for c in swept:
        item = items[c.item]
        n = len(item.data)
        assert len(c.doc) <= 3 * T, c.name
        assert c.doc[c.first:c.last + 1] == item.data and c.last - c.first + 1 == n, c.name
        suffix = dict(E.SUFFIXES)[c.suffix]
        assert c.doc[c.last + 1:] == suffix and c.suffix in item.suffixes, c.name
        pre = c.doc[:c.first]
        if c.prefix == "plain":
            assert pre == b"x" * c.first, c.name
        elif c.prefix == "space":
            assert pre == b"x" * (c.first - 1) + b" ", c.name
        elif c.prefix == "ws":
            assert pre and O.pp_remove_emoji(pre.decode()) == "", c.name
        elif filt == "html":
            assert pre[:1] == b"<" and b">" not in pre and pre.count(b"<") == 1, c.name
        elif filt == "url":
            assert pre[:8] == b"http://a" and not any(ord(ch) in O.WHITESPACE for ch in pre.decode()), c.name
        else:
            head = {"carried_ws0": " ", "carried_seen": "x "}[c.prefix]
            s = pre.decode()
            assert s.startswith(head) and O.pp_remove_emoji(s) == head.strip(), c.name
            assert all(ch == " " or ord(ch) >= 0x24C2 for ch in s[len(head):]), c.name
        E_ = c.edge
        assert E_ in (T, 2 * T)
        want = {"ends_before": c.last == E_ - 2, "ends_at": c.last == E_ - 1, "straddles": c.first <= E_ - 1 < c.last,
                "begins_at": c.first == E_, "begins_after": c.first == E_ + 1}
        assert want[c.kind] and sum(want.values()) == 1, (c.name, c.kind)
        have[(c.item, E_, c.prefix, c.suffix, c.first)] += 1
    # every item x edge x offset x prefix x suffix of the docstring exists, once; nothing else does
    expect = 0
    for item in E.ITEMS[filt]:
        n = len(item.data)
        for edge in (T, 2 * T):
            offs = item_offsets(n, edge)
            assert offs == list(E.offsets(n, edge)) and offs, item.name
            if n + 1 <= T and edge + 1 + n + 5 <= 3 * T:                      # not clipped: the whole range, all four alignments
                assert offs == list(range(edge - n - 1, edge + 2)) and len(offs) == n + 3 >= 4
            kinds = {E.kind_of(o, o + n - 1, edge) for o in offs}
            if n + 1 <= T and edge + 1 + n + 5 <= 3 * T:
                assert kinds == set(E.KINDS) - ({"straddles"} if n == 1 else set()), item.name
            else:
                assert "straddles" in kinds, item.name
            for o in offs:
                for pname in PREFIX_NAMES[filt]:
                    if o < prefix_min(filt, pname):
                        continue
                    for sname in item.suffixes:
                        assert have[(item.name, edge, pname, sname, o)] == 1, (item.name, edge, pname, sname, o)
                        expect += 1
    assert len(swept) == expect == sum(have.values())
    assert len(E.cases(filt)) - len(swept) == FIXED[filt]
    for c in E.cases(filt):
        if c.kind == "fixed":
            assert c.doc[c.first:c.last + 1] and 0 <= c.first <= c.last < len(c.doc) <= 3 * T + 2, c.name


def test_the_issue_s_items_are_there():
    """The minimum list, by content."""
    data = {f: {i.data for i in E.ITEMS[f]} for f in E.FILTERS}
    for s in ("<b>", "<>", "<" + "q" * 70 + ">", "a>b", "<a<b>", "<a>x<b", "<a", "<" + "q" * 63 + ">", "<" + "q" * 127 + ">", "<a><b>", "<a\nb>"):
        assert s.encode() in data["html"], s
    c = lambda *points: "".join(chr(p) for p in points)
    nbsp, ideo, heart, grin, acute = c(0xA0), c(0x3000), c(0x2764), c(0x1F600), c(0x301)
    for s in ("http", "http ", "http" + nbsp, "http" + ideo, "httpy", "http" + c(0xE9), "http" + c(0x1EC7), "http" + grin, "xhttpy",
              "httphttp://a", "http http://a"):
        assert s.encode() in data["url"], s
    for w in (" ", nbsp, ideo):
        assert any(d.startswith(b"http://") and d.endswith((w + "K").encode()) and len(d) < T for d in data["url"])       # over one edge
        assert any(d.startswith(b"http://") and d.endswith((w + "K").encode()) and len(d) > T + 8 for d in data["url"])   # over two
    assert {c.encode() for c in string.punctuation} | {bytes([b]) for b in (0x20, 0x30, 0x39, 0x41, 0x5A, 0x61, 0x7A, 0x7F)} == data["punct"]
    for s in (heart, grin, c(0x200D), c(0x231A), c(0x24C1), c(0x24C2), " ", nbsp, ideo, " " + heart + " ", heart + " " + grin,
              "a" + " " * T + "b", "a" + " " * (T + 1) + "b", "a " + heart * 22 + "b", " ! "):
        assert s.encode() in data["emoji"], s
    for s in ("a" + acute, c(0xE2) + acute, c(0x1B0) + c(0x323), "x" + acute, "a" + acute + acute, "aa" + acute, "a" + c(0x302)):
        assert s.encode() in data["unicode"], s
    table = {c.doc[c.first:c.last + 1].decode(): c for c in E.cases("unicode") if c.item.startswith("table_")}
    assert set(table) == {b + m for b in O._PP_BASES for m in O._PP_MARKS} and len(table) == 120
    for pair, c in table.items():
        assert (c.first + len(pair[0].encode())) % T == 0, c.name                  # the base ends a trip, the mark opens the next
    assert {len(O.COMPOSE[(p[0], p[1])].encode()) for p in table} == {2, 3}
    # the fixed cases that need byte 0: a URL, a mark, deleted + whitespace + deleted
    assert any(c.doc.startswith(b"http://a") for c in E.cases("url") if c.kind == "fixed")
    assert any(c.doc.startswith(E.ACUTE) for c in E.cases("unicode") if c.kind == "fixed")
    assert any(c.doc.startswith(E.HEART + b" " + E.GRIN) for c in E.cases("emoji") if c.kind == "fixed")
    # base + mark as the document's last 3 and 4 bytes, a mark as its last 2
    ends = {c.item for c in E.cases("unicode") if c.suffix == "end"}
    assert {"a_acute", "acirc_acute", "mark_alone"} <= ends


def test_case_counts(capsys):
    total = 0
    for f in E.FILTERS:
        n = len(E.cases(f))
        with capsys.disabled():
            print("\n[preprocess_edges] %-8s %6d cases, %7d bytes" % (f, n, sum(len(c.doc) for c in E.cases(f))), end="")
        assert n == MEASURED[f], (f, n)
        total += n
    for chain, over in E.SWEEPS:
        n = len(E.sweep_cases(over))
        with capsys.disabled():
            print("\n[preprocess_edges] %-32s %6d cases" % (E.chain_id(chain), n), end="")
        assert n == sum(MEASURED[f] for f in over) <= total == 24834
    assert [len(c) for c, _ in E.SWEEPS].count(3) == 1 and {len(c) for c, _ in E.SWEEPS} == {1, 2, 3, 5}
    assert max(len(c.doc) for f in E.FILTERS for c in E.cases(f) if c.kind != "fixed") <= 3 * T


@pytest.mark.parametrize("filt", E.FILTERS)
def test_cases_fire_or_must_not(filt):
    """Under the oracle's filter alone: a "fires" case changes, a "must not fire" case does not; both kinds at both edges."""
    seen = collections.Counter()
    for c in E.cases(filt):
        s = E.text_of(c.doc)
        out = O.PP_OPS[filt](s)
        if c.fires is True:
            assert out != s, c.name
        elif c.fires is False:
            assert out == s, c.name
        if c.fires is not None and c.edge is not None:
            seen[(c.fires, c.edge)] += 1
            for k in E.KINDS:
                seen[(c.fires, c.edge, k)] += c.kind == k
    for fires in (True, False):
        for edge in (T, 2 * T):
            assert seen[(fires, edge)] > 0, (filt, fires, edge)
            assert seen[(fires, edge, "ends_at")] and seen[(fires, edge, "begins_at")], (filt, fires, edge)
    # the must-not-fire items of the issue
    quiet = {c.item for c in E.cases(filt) if c.fires is False}
    assert {"html": {"lone_gt"}, "url": {"http_sp", "http_nbsp", "http_ideo", "http_end"}, "punct": {"border_%02X" % b for b in E.BORDERS},
            "emoji": {"kept_24C1"}, "unicode": {"x_acute", "a_circumflex_mark"}}[filt] <= quiet


def test_the_oracle_against_its_regular_expressions():
    """gz_oracle.py restates the reference's filters as explicit scans; here the patterns themselves, on every case without a
    surrogate (Python's re and str.split see a lone surrogate like any other code point, but the patterns are quoted for text)."""
    table = str.maketrans("", "", string.punctuation)
    n = 0
    for f in E.FILTERS:
        for c in E.cases(f):
            s = E.text_of(c.doc)
            if any(0xD800 <= ord(ch) <= 0xDFFF for ch in s):
                continue
            n += 1
            assert O.pp_remove_html(s) == re.sub(r"<[^>]*>", "", s), c.name
            assert O.pp_remove_url(s) == re.sub(r"http\S+", "", s), c.name
            assert O.pp_remove_punctuations(s) == s.translate(table), c.name
            kept = "".join(ch for ch in s if not any(a <= ord(ch) <= b for a, b in O.EMOJI_RANGES))
            assert O.pp_remove_emoji(s) == " ".join(kept.split()), c.name
    assert n > 24000


def test_probes():
    """Each probe holds the byte or the word its skip test looks for exactly where the name says; "fires" by the oracle."""
    ps = E.probes()
    assert len({p.name for p in ps}) == len(ps)
    for p in ps:
        s = E.text_of(p.doc)
        assert (O.PP_OPS[p.filt](s) != s) == p.fires, p.name
        assert len(p.doc) <= 16
    for i in range(12):
        d = next(p for p in ps if p.name == "http_at_%d" % i).doc
        assert len(d) == i + 5 and d.find(b"http") == i and d[-1:] == b"x"
    for length in range(1, 13):
        for k in range(1, 5):
            if length >= k:
                d = next(p for p in ps if p.name == "lt_last_%d_of_%d" % (k, length)).doc
                assert len(d) == length and d.find(b"<") == length - k
        for k in (2, 3, 4):
            if length >= k + 1:
                d = next(p for p in ps if p.name == "mark_last_%d_of_%d" % (k, length)).doc
                assert len(d) == length and d.find(b"\xcc") == length - k and d[length - k - 1:length - k] == b"a"
    # what the skip tests look for is still there in the cut forms that keep it, and gone where the cut took it
    assert all(b"http" in p.doc for p in ps if p.filt == "url")
    assert all((b"<" in p.doc) == (not p.name.startswith("lt_last_1_")) for p in ps if p.filt == "html" and p.name.endswith("_cut"))


def test_pack_batches():
    batches = E.pack_batches()
    assert tuple(batches) == (1, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025)
    lens = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257)
    for n, docs in batches.items():
        assert len(docs) == n and max(len(d) for d in docs) <= 262 == E.PACK_MAX_DOC
        out = [O.preprocess(d.decode(), ["punct"]) for d in docs]
        assert [len(o) for o in out] == [lens[d % 14] for d in range(n)]
        assert all(0 <= len(d) - len(o) <= 5 and d.startswith(o.encode()) for d, o in zip(docs, out))
        if n >= 33:
            assert {len(d) - len(o) for d, o in zip(docs, out)} == set(range(6))
        if n >= 1023:
            src = dst = 0
            mutual = set()
            for d, o in zip(docs, out):
                mutual.add((src - dst) % 16)
                src, dst = src + len(d), dst + len(o)
            assert mutual == set(range(16))
    # a byte copied from another document or another place of its own is seen: no two 16-byte windows of the large batch agree
    docs = batches[1025]
    wins = collections.Counter(d[i:i + 16] for d in docs for i in range(0, len(d.rstrip(b"!")) - 15))
    assert max(wins.values()) == 1


def test_the_long_document():
    d = E.long_document()
    assert len(d) == 4097 + T > 4096
    s = d.decode()
    for f in E.FILTERS:
        assert O.PP_OPS[f](s) != s, f
    for item in (b"<b>", b"http://ab", b"!?", E.HEART, b"a" + E.ACUTE, E.ACIRC + E.ACUTE, E.GRIN):
        at = d.find(item)
        assert at // T != (at + len(item) + (4 if item == b"http://ab" else 0) - 1) // T, item          # it straddles a trip edge
