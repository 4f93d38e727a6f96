"""The text pre-pass (csrc/gz_preproc.inc) at the trip edges of pp_filter, byte for byte against oracle/gz_oracle.py: preprocess.

The documents come from tests/preprocess_edges.py (tests/test_preprocess_edges_inputs.py proves on the CPU that each sits on its edge
and that the oracle agrees with the reference's regular expressions on all of them).  Every batch runs on three paths:

  fused   a context with defaults: gz_pp_fused_kernel runs the whole chain on chip (LDS reads, the skip tests, punct + emoji as one
          pass), gz_scan32m_kernel + gz_pp_pack4_kernel pack the result
  chain   a context with pp_fused = 0: gz_pp_kernel filter by filter through the slot buffers (unaligned global loads),
          gz_launch_scan64 + gz_pp_pack_kernel
  mixed   the default context and one document of 4 097 + 64 bytes behind, then in front of, the batch: the short documents on chip,
          the long one by the chain, both out of the slot buffer the two kernels must agree on ((n_ops - 1) & 1)

Text filters: no tolerance anywhere."""
import contextlib

import numpy as np
import pytest

import gz_oracle as O
import preprocess_edges as E

pytestmark = pytest.mark.gpu

PATHS = ("fused", "chain", "mixed")
_WANT = {}


def want_of(chain, docs):
    """the oracle's outputs (bytes), computed once per chain and document"""
    memo = _WANT.setdefault(tuple(chain), {})
    out = []
    for d in docs:
        w = memo.get(d)
        if w is None:
            w = memo[d] = E.u(O.preprocess(E.text_of(d), list(chain)))
        out.append(w)
    return out


@pytest.fixture(scope="module")
def ctx():
    from genz_tokenize import _native
    c = _native.Context()
    try:
        yield c
    finally:
        c.close()


@contextlib.contextmanager
def chain_context():
    from genz_tokenize import _native
    c = _native.Context()
    try:
        _native.debug_set("pp_fused", 0, c)
        yield c
    finally:
        c.close()


def compare(chain, path, names, docs, want, out, oo):
    """per document, and the offsets: oo[0] == 0, differences = the oracle's byte lengths"""
    oo = np.asarray(oo, np.int64)
    assert len(oo) == len(docs) + 1 and oo[0] == 0, (chain, path)
    raw = np.asarray(out, np.uint8).tobytes()
    if np.array_equal(np.diff(oo), [len(w) for w in want]) and raw == b"".join(want):
        return
    bad = []
    for i, w in enumerate(want):
        got = raw[int(oo[i]):int(oo[i + 1])]
        if got != w:
            at = next((k for k in range(min(len(got), len(w))) if got[k] != w[k]), min(len(got), len(w)))
            bad.append("%s: first difference at output byte %d; input %r\n      got  %r\n      want %r" % (names[i], at, docs[i], got, w))
    assert bad, (chain, path, "offsets differ", oo[-1], len(raw))
    pytest.fail("chain %s, path %s: %d of %d documents differ\n  " % (E.chain_id(chain), path, len(bad), len(docs)) + "\n  ".join(bad[:12]))


def run(chain, path, names, docs, ctx):
    from genz_tokenize import preprocess as P
    want = want_of(chain, docs)
    if path == "fused":
        assert max(len(d) for d in docs) <= 4096
        compare(chain, path, names, docs, want, *P.preprocess_packed(*E.pack(docs), list(chain), ctx))
    elif path == "chain":
        with chain_context() as c:
            compare(chain, path, names, docs, want, *P.preprocess_packed(*E.pack(docs), list(chain), c))
    else:
        long = E.long_document()
        assert len(long) > 4096
        wl = want_of(chain, [long])
        compare(chain, "mixed, long document last", names + ["long"], docs + [long], want + wl,
                *P.preprocess_packed(*E.pack(docs + [long]), list(chain), ctx))
        compare(chain, "mixed, long document first", ["long"] + names, [long] + docs, wl + want,
                *P.preprocess_packed(*E.pack([long] + docs), list(chain), ctx))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chain,over", E.SWEEPS, ids=[E.chain_id(c) for c, _ in E.SWEEPS])
def test_sweep(ctx, chain, over, path):
    """Every item of the chain's filters at every offset around the trip edges T and 2 T, behind every prefix, with and without a kept
    character behind it: the carried flags of pp_filter (in_tag, open_abs and the unclosed pass; url_del and c_ws; seen, pend, c_del, c_ws
    and the carry out of bit 63; c_del and the look-back of convert_unicode) in all three instantiations."""
    cs = E.sweep_cases(over)
    run(chain, path, [c.name for c in cs], [c.doc for c in cs], ctx)


@pytest.mark.parametrize("path", ("fused", "chain"))
def test_skip_probes(ctx, path):
    """ppf_has_http and ppf_has_byte must say yes: 'http' at every dword phase with its fifth byte the document's last, '<' and a
    mark's 0xCC among the last four bytes of documents of 1 .. 12 bytes -- and the same documents cut short."""
    ps = E.probes()
    for chain in (("html",), ("unicode",), ("url",), E.ALL5):
        run(chain, path, [p.name for p in ps], [p.doc for p in ps], ctx)


@pytest.mark.parametrize("n_docs", E.PACK_NDOCS)
def test_pack_tail(ctx, n_docs):
    """gz_pp_pack4_kernel (8 lanes a document, 16 bytes a lane and step, 8 documents a wave) and the scans in front of it at document
    counts around a wave, a workgroup and a scan block, output lengths around 16 and 128 bytes, source and destination at every mutual
    alignment; the general tail of the chain path; and the device form with absolute offsets into an output of exactly `total` bytes."""
    docs = E.pack_batches()[n_docs]
    names = ["doc %d" % d for d in range(n_docs)]
    chain = ("punct",)
    run(chain, "fused", names, docs, ctx)
    run(chain, "chain", names, docs, ctx)
    want = b"".join(want_of(chain, docs))
    total = len(want)
    text, off = E.pack(docs)
    nbytes = int(off[-1])
    junk, guard = 37, 64
    bufs = [ctx.alloc(junk + nbytes + 64), ctx.alloc(8 * (n_docs + 1)), ctx.alloc(guard + total + guard), ctx.alloc(8 * (n_docs + 1))]
    try:
        d_text, d_off, d_out, d_oo = bufs
        ctx.h2d(d_text, np.concatenate([np.full(junk, 0x21, np.uint8), text, np.full(64, 0x21, np.uint8)]))     # ('!' all around)
        ctx.h2d(d_off, off + junk)
        ctx.h2d(d_out, np.full(guard + total + guard, 0xA5, np.uint8))
        got_total = ctx.preprocess_device([3], d_text, d_off, n_docs, nbytes, d_out + guard, total, d_oo)
        got = np.empty(guard + total + guard, np.uint8); ctx.d2h(got, d_out)
        oo = np.empty(n_docs + 1, np.int64); ctx.d2h(oo, d_oo)
    finally:
        for b in bufs:
            ctx.free(b)
    assert got_total == total == int(oo[n_docs])
    assert np.all(got[:guard] == 0xA5) and np.all(got[guard + total:] == 0xA5)
    compare(chain, "device form", names, docs, want_of(chain, docs), got[guard:guard + total], oo)


def test_single_call_names_at_the_edge():
    """remove_html, convert_unicode, remove_punctuations, remove_emoji and remove_URL: the module-level context, a batch of one."""
    from genz_tokenize import preprocess as P
    fns = {"html": P.remove_html, "unicode": P.convert_unicode, "punct": P.remove_punctuations, "emoji": P.remove_emoji, "url": P.remove_URL}
    for f, fn in fns.items():
        edge = "ends_at" if f == "punct" else "straddles"          # (a one-byte item cannot straddle)
        cs = [c for c in E.cases(f) if c.kind == edge and c.fires and c.suffix == "tail"]
        picked = [cs[0], cs[len(cs) // 2], cs[-1]]
        assert len({c.name for c in picked}) == 3
        for c in picked:
            s = E.text_of(c.doc)
            assert fn(s) == O.preprocess(s, [f]) != s, c.name
