"""A gzip GFA inflated and split on the device (phi_gfa_gzip_split): the split against a restatement of the
host reader's line rules, offsets beyond 4 GiB, the graphs it gives against the host reader's, the statuses it refuses
with, and the command line's route (PHI_GFA_INFLATE_MIN) against the host reader's run (PHI_GFA_INFLATE=0)."""
import ctypes as C
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import DATA, ROOT
from test_cpu_gfa_gzip import split_rule

pytestmark = pytest.mark.gpu

HEAD = b"S\t1\tACGT\nS\t2\tGG\nS\t3\tT\nL\t1\t+\t2\t+\t0M\nL\t2\t+\t3\t+\t0M\n"


def _ctx(ctx_factory):
    return ctx_factory(k=3, w=2, threshold=1.0, recombination=100)


def _walk(steps, tags=b""):
    return b"".join(b">%d" % s for s in steps) + tags


def _edge_texts():
    t = {}
    t["crlf, no final newline"] = HEAD + b"W\tA\t1\tc\t0\t6\t>1>2\r\nW\tB\t2\tc\t0\t6\t>1>2>3"
    t["W-line first and last"] = b"W\tA\t1\tc\t0\t6\t>1\n" + HEAD + b"W\tB\t1\tc\t0\t6\t>2>3\n"
    t["5 tabs, no tab, Wx"] = HEAD + b"W\tA\t1\tc\t0\t>1>2\nW\nW\t\nWx\tA\t1\tc\t0\t6\t>1\nW\tB\t1\tc\t0\t6\t>1>2\n"
    t["empty walk, tags"] = HEAD + b"W\tA\t1\tc\t0\t6\t\nW\tB\t1\tc\t0\t6\t>1>2>3\tTG:Z:x\tXY:i:3\r\n"
    t["a last line of '\\r'"] = HEAD + b"W\tA\t1\tc\t0\t6\t>1>2\r"
    t["across many tiles"] = HEAD + b"W\tA\t1\tc\t0\t6\t" + _walk([1, 2, 3] * 120_000) + b"\nW\tB\t1\tc\t0\t6\t>1\n"
    for shift in range(4):                                   # "\nW\t" straddling the 64-KB border at each of its bytes
        pad = (1 << 16) - len(HEAD) - 3 - 1 + shift
        t[f"straddle {shift}"] = HEAD + b"#" + b"x" * pad + b"\nW\tA\t1\tc\t0\t6\t>1>2\n" + b"W\tB\t1\tc\t0\t6\t>3\n"
    return t


@pytest.mark.parametrize("name", list(_edge_texts()))
def test_split_follows_the_host_readers_rules(ctx_factory, name):
    text = _edge_texts()[name]
    want_host, walks = split_rule(text)
    ctx = _ctx(ctx_factory)
    for gz in (gzip.compress(text, 6), gzip.compress(text[: len(text) // 2], 1) + gzip.compress(text[len(text) // 2:], 9)):
        host, info = ctx.gfa_gzip_split(gz)
        assert host == want_host, name
        assert info["n_walks"] == len(walks) and info["walk_bytes"] == sum(e - b for b, e in walks)
        assert info["text_bytes"] == len(text) and info["host_bytes"] == len(host)
    # the walk fields left on the device are the ones an upload sends: the same entries once resolved
    if walks:
        w1, flag1 = _resolve(ctx, len(walks), [-1, 0, 1, 2])
        got = ctx.walk_entries() if not flag1 else None
        bufs = [C.create_string_buffer(text[b:e], e - b) for b, e in walks]
        arr = (C.c_int64 * (2 * len(walks)))(*[v for (b, e), s in zip(walks, bufs) for v in (C.addressof(s), e - b)])
        ctx._chk(ctx._L.phi_walk_text_upload(ctx._h, arr, len(walks)))
        w2, flag2 = _resolve(ctx, len(walks), [-1, 0, 1, 2])
        assert flag1 == flag2
        if not flag1:
            assert np.array_equal(w1, w2) and np.array_equal(got, ctx.walk_entries())


def _resolve(ctx, n_walks, num2id):
    """phi_walk_text_resolve over names <number> -> num2id[number]: (walk offsets, irregular)"""
    n2i = np.array(num2id, np.int32)
    woff = np.zeros(n_walks + 1, np.int64)
    flag = C.c_uint32()
    ctx._chk(ctx._L.phi_walk_text_resolve(ctx._h, b"", 0, n2i.ctypes.data, len(n2i), int(n2i.max()) + 1, woff.ctypes.data, C.byref(flag)))
    return woff, flag.value


def test_offsets_beyond_4_gib(ctx_factory):
    """a walk field whose tags run past 2^32 bytes, then a second W-line behind 2^32: concatenated members of one repeated
    block (the device holds the text, its tiles and the inflater's working set at once: ~25 GB)"""
    block = b"x" * (64 << 20)
    head = b"S\t1\tA\nS\t2\tC\nL\t1\t+\t2\t+\t0M\nW\tA\t1\tc\t0\t6\t>1>2\tXX:Z:"
    tail = b"\nW\tB\t1\tc\t0\t6\t>2\n"
    k = (4 << 30) // len(block) + 1
    member = gzip.compress(block, 9)
    gz = gzip.compress(head, 6) + member * k + gzip.compress(tail, 6)
    n = len(head) + k * len(block) + len(tail)
    ctx = _ctx(ctx_factory)
    host, info = ctx.gfa_gzip_split(gz)
    first = len(head) - len(b">1>2\tXX:Z:")
    assert info["text_bytes"] == n and info["n_walks"] == 2
    assert host == head[:first] + b"\nW\tB\t1\tc\t0\t6\t\n"
    assert info["walk_bytes"] == (n - len(tail) - first) + 2
    woff, flag = _resolve(ctx, 2, [-1, 0, 1])
    assert flag == 0 and woff.tolist() == [0, 2, 3]
    assert ctx.walk_entries().tolist() == [0, 1, 1]


def _same_as_host_reader(g, want, ctx):
    assert g.route == "device" and g.walk_vtx is None
    assert g.hap_id2name == want.hap_id2name
    for f in ("seq_off", "adj_off", "adj", "top_order_map", "walk_off"):
        assert np.array_equal(getattr(g, f), getattr(want, f)), f
    assert bytes(g.seq_concat) == bytes(want.seq_concat)
    assert np.array_equal(ctx.walk_entries(), want.walk_vtx)


def test_mhc4_through_the_device_route(ctx_factory):
    from phi_amd import ilp_index as H
    path = os.path.join(DATA, "MHC_4.gfa.gz")
    ctx = _ctx(ctx_factory)
    g = H.DeferredGraph.from_gzip_on_device(path, ctx)
    want = H.Graph(path)
    _same_as_host_reader(g, want, ctx)
    assert g.split_info["n_walks"] == want.num_walks
    assert g.split_info["host_bytes"] + g.split_info["walk_bytes"] == g.split_info["text_bytes"]
    # and the same walk entries as the upload of the reader's own walk fields
    ref = H.DeferredGraph(path)
    assert ref.resolve_on_device(ctx)
    assert np.array_equal(ctx.walk_entries(), want.walk_vtx) and np.array_equal(ref.walk_off, g.walk_off)


def test_c2_size_synthetic_graph(ctx_factory, tmp_path):
    from phi_amd import ilp_index as H
    from phi_amd import synth
    s = synth.NativeGraph(backbone_len=5_000_000, n_walks=49, seed=4901)
    plain = str(tmp_path / "c2.gfa")
    s.write_gfa(plain)
    s.close()
    text = open(plain, "rb").read()
    path = str(tmp_path / "c2.gfa.gz")
    with open(path, "wb") as f:
        f.write(gzip.compress(text, 1))
    ctx = _ctx(ctx_factory)
    g = H.DeferredGraph.from_gzip_on_device(path, ctx)
    want = H.Graph(plain)
    _same_as_host_reader(g, want, ctx)
    assert g.split_info["text_bytes"] == len(text)


def test_bad_inputs_get_their_status_and_the_context_stays_usable(ctx_factory, tmp_path):
    from phi_amd import PHI_ERR_INVALID, PHI_ERR_UNSUPPORTED, PhiError
    from phi_amd import ilp_index as H
    good = open(os.path.join(DATA, "MHC_4.gfa.gz"), "rb").read()
    bad = bytearray(good)
    bad[-6] ^= 0x40                                          # the trailer's CRC32
    ctx = _ctx(ctx_factory)
    for data in (bytes(bad), good[: len(good) // 2], good[:5]):
        with pytest.raises(PhiError) as e:
            ctx.gfa_gzip_split(data)
        assert e.value.status == PHI_ERR_INVALID
    # BGZF is gzip (members with an extra field): the split takes it as any multi-member stream; the command line leaves it
    # to the host pool
    text = gzip.decompress(good)
    bgzf = b"".join(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00\x00\x00" + zlib.compress(text[i:i + 65280], 6)[2:-4]
                    + zlib.crc32(text[i:i + 65280]).to_bytes(4, "little") + len(text[i:i + 65280]).to_bytes(4, "little")
                    for i in range(0, len(text), 65280))
    host, info = ctx.gfa_gzip_split(bgzf)
    assert host == split_rule(text)[0]
    # more W-lines than the list holds: refused, nothing kept
    os.environ["PHI_GFA_SPLIT_CAP"] = "2"
    try:
        with pytest.raises(PhiError) as e:
            ctx.gfa_gzip_split(good)
        assert e.value.status == PHI_ERR_UNSUPPORTED
    finally:
        del os.environ["PHI_GFA_SPLIT_CAP"]
    g = H.DeferredGraph.from_gzip_on_device(os.path.join(DATA, "MHC_4.gfa.gz"), ctx)
    _same_as_host_reader(g, H.Graph(os.path.join(DATA, "MHC_4.gfa.gz")), ctx)


# ---- the command line

PHI = os.path.join(ROOT, "phi_amd", "PHI")
GFA = os.path.join(DATA, "MHC_4.gfa.gz")
READS = os.path.join(DATA, "CHM13_reads.fq.gz")
DEVICE = {"PHI_TIMING": "1", "PHI_GFA_INFLATE_MIN": "0", "PHI_READ_CHUNK": "100000"}
HOST = {"PHI_TIMING": "1", "PHI_GFA_INFLATE": "0", "PHI_READ_CHUNK": "100000"}


def run(args, cwd, env):
    if not os.path.exists(PHI):
        import __graft_entry__
        __graft_entry__.build()
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([PHI] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300, env=e)


def lines(log):
    return [re.sub(r"^\[M::[^\]]*\] ", "", l) for l in log.splitlines()
            if not (l.startswith("[phi timing]") or "Real time" in l or "CMD:" in l or "written to" in l)]


def fasta(path):
    return path.read_text().split("\n")[1:]


def on_device(log):
    return re.search(r"\[phi timing\] main: GFA: (\d+) bytes inflated on the device from (\d+) gzip bytes .*; (\d+) bytes to the host, (\d+) bytes of (\d+) walks kept", log)


def single_stream(tmp_path):
    """the fixture MHC_4.gfa.gz is BGZF (the host pool's, whatever the threshold): its text as one gzip member"""
    path = tmp_path / "MHC_4.gfa.gz"
    path.write_bytes(gzip.compress(gzip.decompress(open(GFA, "rb").read()), 6))
    return str(path)


def test_golden_graph_through_the_device(tmp_path):
    gfa = single_stream(tmp_path)
    host = run(["-t8", "-g", gfa, "-r", READS, "-o", str(tmp_path / "host.fa")], tmp_path, HOST)
    dev = run(["-t8", "-g", gfa, "-r", READS, "-o", str(tmp_path / "dev.fa")], tmp_path, DEVICE)
    assert host.returncode == 0 and dev.returncode == 0, host.stderr[-2000:] + dev.stderr[-2000:]
    m = on_device(dev.stderr)
    assert m and int(m.group(1)) == 13_996_110 and int(m.group(5)) == 5, dev.stderr[-3000:]
    assert int(m.group(3)) + int(m.group(4)) == 13_996_110
    assert not on_device(host.stderr) and "GFA: not on the device" not in host.stderr
    assert lines(host.stderr) == lines(dev.stderr)
    assert fasta(tmp_path / "host.fa") == fasta(tmp_path / "dev.fa")
    # below the threshold (the default 16 MB): today's path
    default = run(["-t8", "-g", gfa, "-r", READS, "-o", str(tmp_path / "default.fa")], tmp_path, {"PHI_TIMING": "1", "PHI_READ_CHUNK": "100000"})
    assert default.returncode == 0 and not on_device(default.stderr)
    # BGZF keeps the host pool
    bgzf = run(["-t8", "-g", GFA, "-r", READS, "-o", str(tmp_path / "bgzf.fa")], tmp_path, DEVICE)
    assert bgzf.returncode == 0 and not on_device(bgzf.stderr) and "GFA: not on the device" not in bgzf.stderr


def test_both_gzip_routes_and_several_jobs(tmp_path):
    text = gzip.open(READS, "rb").read()
    recs = text.split(b"\n")
    half = (len(recs) // 8) * 4
    (tmp_path / "b.fq.gz").write_bytes(gzip.compress(b"\n".join(recs[half:]), 6))
    jobs = ["-r", READS, "-o", "a.fa", "-r", str(tmp_path / "b.fq.gz"), "-o", "b.fa"]
    (tmp_path / "h").mkdir()
    (tmp_path / "d").mkdir()
    gfa = single_stream(tmp_path)
    host = run(["-t8", "-g", gfa] + jobs, tmp_path / "h", dict(HOST, PHI_INFLATE="0"))
    dev = run(["-t8", "-g", gfa] + jobs, tmp_path / "d", dict(DEVICE, PHI_INFLATE_MIN="0"))
    assert host.returncode == 0 and dev.returncode == 0, host.stderr[-2000:] + dev.stderr[-2000:]
    assert on_device(dev.stderr) and re.search(r"main: \d+ bytes inflated on the device from", dev.stderr)
    assert lines(host.stderr) == lines(dev.stderr)
    for f in ("a.fa", "b.fa"):
        assert fasta(tmp_path / "h" / f) == fasta(tmp_path / "d" / f)


def _fallback_files(tmp_path):
    text = gzip.decompress(open(GFA, "rb").read())
    s_end = text.index(b"\nW\t") + 1
    w_end = text.index(b"\n", s_end) + 1
    f = {}
    # a W-line among the S-lines: the first walk moved in front of the last S-line
    s_last = text.rindex(b"\nS\t", 0, s_end) + 1
    f["W-line among the S-lines"] = text[:s_last] + text[s_end:w_end] + text[s_last:s_end] + text[w_end:]
    # names of another form: one segment renamed (its S-line, links and steps)
    name = re.match(rb"S\t(\S+)\t", text[text.index(b"S\t"):]).group(1)
    f["names not <prefix><number>"] = re.sub(rb"(?<=[\t>])" + re.escape(name) + rb"(?=[\t>\n])", b"seg_x" + name, text)
    # a reverse step in a walk
    i = text.index(b">", s_end)
    f["irregular walk text"] = text[:i] + b"<" + text[i + 1:]
    return {k: gzip.compress(v, 1) for k, v in f.items()}


@pytest.mark.parametrize("case", ["W-line among the S-lines", "names not <prefix><number>", "irregular walk text", "gzip stream corrupt"])
def test_fallbacks_give_the_host_readers_output(tmp_path, case):
    if case == "gzip stream corrupt":
        data = bytearray(open(single_stream(tmp_path), "rb").read())
        data[-6] ^= 0x40
        data = bytes(data)
    else:
        data = _fallback_files(tmp_path)[case]
    path = tmp_path / "g.gfa.gz"
    path.write_bytes(data)
    args = ["-t8", "-g", str(path), "-r", READS]
    host = run(args + ["-o", str(tmp_path / "host.fa")], tmp_path, HOST)
    dev = run(args + ["-o", str(tmp_path / "dev.fa")], tmp_path, DEVICE)
    assert host.returncode == dev.returncode, (case, host.returncode, dev.returncode, dev.stderr[-2000:])
    assert lines(host.stderr) == lines(dev.stderr), case
    assert not on_device(dev.stderr)
    assert re.search(r"GFA: not on the device \([^)]*" + re.escape(case), dev.stderr), dev.stderr[-2000:]
    if host.returncode == 0:
        assert fasta(tmp_path / "host.fa") == fasta(tmp_path / "dev.fa")
