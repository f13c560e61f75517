"""The gzip GFA split on the device, checked without a GPU: the new symbols, the splitter's kernel budget, and
the host reader from memory (phi_gfa_read_deferred_text) against the reader from the file, on whole and on split text."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "phi_amd", "csrc", "gfa_text.hip")


def split_rule(text):
    """The host reader's line rules (gfa_reader.cpp scan_slice / split_tabs), restated: lines end at '\\n' (the last may
    lack it), one '\\r' before the end is not part of the line; a line of at least 3 bytes starting "W\\t" is a walk when
    it holds at least 6 tabs, and its walk field is everything after the 6th tab.  Returns (host text, [(b, e)] of the
    walk fields in file order): the host text is the text with every walk field cut out."""
    walks, pos, n = [], 0, len(text)
    while pos < n:
        nl = text.find(b"\n", pos)
        end = nl if nl >= 0 else n
        e = end - 1 if end > pos and text[end - 1] == 0x0D else end
        if e - pos >= 3 and text[pos] == 0x57 and text[pos + 1] == 0x09:
            t, k = pos - 1, 0
            while k < 6:
                t = text.find(b"\t", t + 1, e)
                if t < 0:
                    break
                k += 1
            if k == 6:
                walks.append((t + 1, e))
        pos = end + 1 if nl >= 0 else n
    host, at = [], 0
    for b, e in walks:
        host.append(text[at:b])
        at = e
    host.append(text[at:])
    return b"".join(host), walks


@pytest.fixture(scope="module")
def host():
    import __graft_entry__
    __graft_entry__.ensure_built()
    from phi_amd import ilp_index as H
    return H


def test_symbols_are_exported(host):
    from phi_amd import _capi
    L = _capi.load()
    for name in ("phi_gfa_gzip_split", "phi_gfa_gzip_free"):
        assert name in _capi.SYMBOLS and getattr(L, name)
    assert "phi_gfa_read_deferred_text" in host.HOST_SYMBOLS and host.host_lib().phi_gfa_read_deferred_text
    assert "phi_gfa_gzip_info" in open(os.path.join(ROOT, "include", "phi_amd.h")).read()
    fields = [f for f, _ in _capi.PhiGfaGzipInfo._fields_]
    assert fields == ["text_bytes", "host_bytes", "walk_bytes", "n_walks", "inflate"]


@pytest.fixture(scope="module")
def split_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("asm") / "gfa_text.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), SRC],
                          stderr=subprocess.DEVNULL)
    return out.read_text()


def _meta(asm, name):
    entries = asm.split("  - .agpr_count:")
    hits = [e for e in entries[1:] if re.search(r"\.name:\s+\S*" + re.escape(name), e)]
    assert len(hits) == 1, f"{len(hits)} metadata entries for {name}"
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", hits[0])}


# streaming kernels, eight waves per SIMD at most 64 VGPRs; a word of LDS; no scratch
BUDGET = {"phi_gfa_split_scan_kernel": (64, 64), "phi_gfa_split_line_kernel": (64, 0), "phi_gfa_split_copy_kernel": (32, 0)}


@pytest.mark.parametrize("kernel", list(BUDGET))
def test_split_kernels_stay_within_budget(split_asm, kernel):
    m = _meta(split_asm, kernel)
    vgpr, lds = BUDGET[kernel]
    assert m["vgpr_count"] <= vgpr, m
    assert m["group_segment_fixed_size"] <= lds, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


def _name_index(H, g):
    prefix, pn, tbl, nn = C.c_void_p(), C.c_int32(), C.c_void_p(), C.c_int64()
    if H.host_lib().phi_graph_name_index(g._h, C.byref(prefix), C.byref(pn), C.byref(tbl), C.byref(nn)) != 0:
        return None
    return (C.string_at(prefix, pn.value) if pn.value else b"",
            np.ctypeslib.as_array(C.cast(tbl, C.POINTER(C.c_int32)), (nn.value,)).copy() if nn.value else np.zeros(0, np.int32))


def _walk_texts(g):
    return [C.string_at(a, n) if n else b"" for a, n in g.walk_texts()]


def _same_graph(H, a, b):
    for f in ("n_vtx", "num_walks", "seq_concat", "seq_off", "adj_off", "adj", "top_order_map", "hap_id2name"):
        x, y = getattr(a, f), getattr(b, f)
        assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), f
    ia, ib = _name_index(H, a), _name_index(H, b)
    assert (ia is None) == (ib is None)
    if ia is not None:
        assert ia[0] == ib[0] and np.array_equal(ia[1], ib[1])


def _from_memory(H, text, name):
    buf = C.create_string_buffer(text, len(text))          # (borrowed by the reader: kept alive by the graph object)
    g = H.DeferredGraph(name, _text=(C.addressof(buf), len(text)))
    g._buf = buf
    return g


def _texts():
    yield "test.gfa", open(os.path.join(DATA, "test.gfa"), "rb").read(), os.path.join(DATA, "test.gfa")
    yield "MHC_4.gfa.gz", gzip.open(os.path.join(DATA, "MHC_4.gfa.gz")).read(), os.path.join(DATA, "MHC_4.gfa.gz")


@pytest.mark.parametrize("which", [0, 1])
def test_reader_from_memory_equals_reader_from_file(host, which, tmp_path):
    name, text, path = list(_texts())[which]
    f = host.DeferredGraph(path)
    m = _from_memory(host, text, path)
    _same_graph(host, f, m)
    assert _walk_texts(f) == _walk_texts(m)
    f.resolve_on_host()
    m.resolve_on_host()
    assert np.array_equal(f.walk_off, m.walk_off) and np.array_equal(f.walk_vtx, m.walk_vtx)
    # and the whole graph equals the eager reader's
    g = host.Graph(path)
    assert np.array_equal(g.walk_vtx, m.walk_vtx) and g.hap_id2name == m.hap_id2name


@pytest.mark.parametrize("which", [0, 1])
def test_reader_on_split_text(host, which):
    name, text, path = list(_texts())[which]
    split, walks = split_rule(text)
    f = host.DeferredGraph(path)
    m = _from_memory(host, split, path)
    _same_graph(host, f, m)
    assert len(walks) == f.num_walks == m.num_walks
    assert _walk_texts(m) == [b""] * len(walks)
    assert _walk_texts(f) == [text[b:e] for b, e in walks]
    assert len(split) == len(text) - sum(e - b for b, e in walks)


def test_split_rule_edges(host):
    """the restatement against the reader itself on edge texts: same walks, same walk fields"""
    s = b"S\t1\tACGT\nS\t2\tGG\nL\t1\t+\t2\t+\t0M\n"
    cases = [
        s + b"W\tA\t1\tc\t0\t6\t>1>2\r\nW\tB\t2\tc\t0\t6\t>1>2",                  # CRLF, no final newline
        s + b"W\tA\t1\tc\t0\t6\t>1>2\tTG:Z:x\n" + b"W\tA\t1\tc\t0\n" + b"Wx\t\t\t\t\t\t>1\n" + b"W\n",   # tags, 5 tabs, Wx, no tab
        s + b"W\tA\t1\tc\t0\t6\t\n" + b"W\tB\t1\tc\t0\t6\t>1\r\r\n",                # empty walk field, two '\r'
        s + b"W\tA\t1\tc\t0\t6\t>1>2\r",                                        # a last line ending in '\r'
    ]
    for text in cases:
        split, walks = split_rule(text)
        m = _from_memory(host, text, "edge")
        assert _walk_texts(m) == [text[b:e] for b, e in walks], text
        ms = _from_memory(host, split, "edge")
        assert ms.num_walks == len(walks) and _walk_texts(ms) == [b""] * len(walks)
        assert ms.hap_id2name == m.hap_id2name
