"""GPU tests of the BAM reads route through the C ABI (phi_reads_bam_*, phi_amd/csrc/bam.hip): the reads the device decodes
from an inflated BAM stream (reads_bam_last_batch: bases and offsets) and phi_bam_info against bam_util.decode, the
sequential Python walk of the same bytes, element for element; no tolerance.  Rules from the SAM/BAM specification; nothing
here was compared with samtools.

Shapes: the smallest at which the kernels can go wrong -- l_seq 0, 1, 2, odd, even; names of 1 and 255 bytes; 0 and 65 535
cigar operations; aux data larger than a tile; every combination of 0x10 / 0x100 / 0x800; tiles of 64, 256 and 4 096 bytes
with records that straddle them, a record longer than many tiles and a record that starts exactly on a tile border; the
stream cut into calls of 1, 3, 4, 37 and 1 000 bytes; a false record chain planted at the start of a tile."""
import gzip
import os
import re
import struct

import numpy as np
import pytest

import bam_util as B
from conftest import DATA

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -4


@pytest.fixture(scope="module")
def ctx(ctx_factory, oracle):
    g = oracle.parse_gfa(os.path.join(DATA, "test.gfa"))
    A = g.arrays()
    c = ctx_factory(k=3, w=2, threshold=1.0, recombination=100)
    c.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
    return c


def _records(bases, off):
    raw = bytes(bases)
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def run_stream(ctx, data, call_bytes, tile, max_chunk=1 << 20, park=None):
    """The reads and the info of `data` fed in calls of call_bytes (None: one call); with a park, the second piece of every
    three waits in device memory first."""
    ctx.reset_reads()
    ctx.reads_bam_begin(max_chunk, tile)
    reads = []
    step = call_bytes or len(data)
    for j, i in enumerate(range(0, len(data), step)):
        piece = data[i:i + step]
        if park is not None and j % 3 == 1:
            idx = park.add(piece)
            ctx.add_reads_bam_parked(park, idx)
            park.release(idx)
        else:
            ctx.add_reads_bam(piece)
        reads += _records(*ctx.reads_bam_last_batch())
    return reads, ctx.reads_bam_end()


def check(ctx, data, call_bytes, tile, **kw):
    want, winfo = B.decode(data)
    got, info = run_stream(ctx, data, call_bytes, tile, **kw)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, call_bytes, tile)
    for key, v in winfo.items():
        assert info[key] == v, (key, info, winfo)
    st = ctx.reads_stats()
    assert st["n_reads"] == winfo["n_kept"] and st["n_bases"] == winfo["n_bases"]
    assert info["tiles"] >= info["tiles_confirmed"] + info["tiles_rewalked"]
    return info


def _seq(rng, n, all_codes=False):
    return bytes(rng.choice(np.frombuffer(B.CODES if all_codes else b"ACGT", np.uint8), n))


FLAGS = [f | p for f in (0, 0x10, 0x100, 0x110, 0x800, 0x810, 0x900, 0x910) for p in (0, 0x1 | 0x40, 0x1 | 0x80 | 0x20)]


def small_file(seed=5):
    """Unaligned BAM (n_ref 0), a dozen records: what the 1-, 3- and 4-byte calls walk through."""
    rng = np.random.default_rng(seed)
    recs = [B.record(b"", _seq(rng, 1), flag=4), B.record(b"q", _seq(rng, 2), flag=4 | 0x10), B.record(b"empty", b"", flag=4)]
    for i, n in enumerate((33, 40, 7, 150, 151, 64)):
        recs.append(B.record(b"read%d" % i, _seq(rng, n, all_codes=i % 2 == 0), flag=4 | FLAGS[(5 * i) % len(FLAGS)],
                             aux=B.aux_bytes(b"zq", bytes(rng.integers(0, 256, 3 * i, dtype=np.uint8)))))
    return B.header(b"@HD\tVN:1.6\tSO:unsorted\n") + b"".join(recs)


def main_file(big, seed=11):
    """A few hundred records against a few hundred references; big: with the record of 65 535 cigar operations (262 KB: many
    tiles without a start) and aux data larger than a 4 096-byte tile.  One record starts exactly 8 192 bytes behind the first."""
    rng = np.random.default_rng(seed)
    refs = [(b"chr%d_%s" % (i, b"x" * (i % 17)), 1000 + i) for i in range(300)]
    recs, at = [], 0

    def add(r):
        nonlocal at
        recs.append(r)
        at += len(r)
    add(B.record(b"", _seq(rng, 1), flag=0, ref_id=0, pos=5))
    add(B.record(b"n" * 254, _seq(rng, 2), flag=0x10, ref_id=299, pos=7, n_cigar=1))
    add(B.record(b"none", b"", flag=0, ref_id=3, pos=1))
    for i in range(280):
        n = int(rng.choice([150, 151, 75, 76, 33, 1, 2, 0, 400]))
        f = FLAGS[i % len(FLAGS)]
        n_cigar = int(rng.integers(0, 4))
        aux = B.aux_bytes(b"zz", bytes(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8))) if i % 3 else b""
        if i == 40:
            # the next record begins exactly 8 192 bytes behind the first one: on a border of every tile size used
            fixed = 4 + 32 + 5 + 4 * n_cigar + (n + 1) // 2 + n + 8
            aux = B.aux_bytes(b"pd", bytes((-(at + fixed)) % 8192))
        add(B.record(b"r%03d" % i, _seq(rng, n, all_codes=i % 5 == 0), flag=f, ref_id=int(rng.integers(-1, 300)), pos=int(rng.integers(0, 1000)),
                     n_cigar=n_cigar, next_ref=int(rng.integers(-1, 300)), aux=aux))
        if i == 40:
            assert at % 8192 == 0
        if big and i == 100:
            add(B.record(b"cigars", _seq(rng, 151), flag=0x10, ref_id=1, pos=2, n_cigar=65535))
        if big and i == 200:
            add(B.record(b"bigaux", _seq(rng, 150), flag=0, ref_id=2, pos=3, aux=B.aux_bytes(b"zb", bytes(rng.integers(0, 256, 9000, dtype=np.uint8)))))
    return B.header(b"@HD\tVN:1.6\n@CO\t" + b"c" * 700 + b"\n", refs) + b"".join(recs)


@pytest.fixture(scope="module")
def files():
    return dict(small=small_file(), main=main_file(False), big=main_file(True))


@pytest.mark.parametrize("tile", [64, 256, 4096])
def test_tiles_of_every_size_over_the_whole_file(ctx, files, tile):
    """One call, the library's own cutting (max_chunk below the file's size for the big one): records straddle tile borders,
    262 KB of cigar and 9 KB of aux leave tiles without a start, one record starts exactly on a border."""
    info = check(ctx, files["main"], None, tile)
    assert info["n_ref"] == 300 and info["tiles_rewalked"] <= info["tiles"]
    want, winfo = B.decode(files["big"])
    ctx.reset_reads()
    ctx.reads_bam_begin(200_000, tile)                         # (pieces of 200 000 bytes: the 262 KB record spans two of them)
    ctx.add_reads_bam(files["big"])
    info = ctx.reads_bam_end()
    st, hits = ctx.reads_stats(), _hits(ctx)
    assert (st["n_reads"], st["n_bases"]) == (winfo["n_kept"], winfo["n_bases"])
    for key, v in winfo.items():
        assert info[key] == v, (key, info, winfo)
    check(ctx, files["big"], None, tile, max_chunk=1 << 20)   # ... and in one piece, read for read
    # (reads_bam_last_batch shows the last piece only: what the pieces cut inside the library gave is compared through the
    #  read state -- minimisers emitted, distinct ones, hit vector -- with the one-piece run, whose reads were compared)
    assert st == ctx.reads_stats() and st["n_emitted"] > 100 and np.array_equal(hits, _hits(ctx)) and hits.any()


@pytest.mark.parametrize("call", [1, 3, 4])
def test_calls_of_a_few_bytes(ctx, files, call):
    """Every field of every record -- block_size and the fixed part among them -- is split at every offset by the 1-byte calls."""
    check(ctx, files["small"], call, 64)


def test_the_cut_of_the_library_made_by_the_caller_read_for_read(ctx, files):
    """The pieces bam_piece sees when the library cuts a call at max_chunk_bytes = 200 000 are those of calls of 200 000 bytes
    behind the header: the same cuts made by the caller, where every piece's batch can be read back."""
    hdr = B.parse_header(files["big"])[0]
    data = files["big"]
    want, winfo = B.decode(data)
    ctx.reset_reads()
    ctx.reads_bam_begin(200_000, 256)
    ctx.add_reads_bam(data[:hdr])
    got = []
    for i in range(hdr, len(data), 200_000):
        ctx.add_reads_bam(data[i:i + 200_000])
        got += _records(*ctx.reads_bam_last_batch())
    info = ctx.reads_bam_end()
    assert got == want and info["n_records"] == winfo["n_records"]


@pytest.mark.parametrize("call,tile", [(37, 256), (1000, 64), (1000, 4096)])
def test_calls_of_37_and_1000_bytes(ctx, files, call, tile):
    """The header (300 references, 7 KB) is longer than the first pieces."""
    assert B.parse_header(files["main"])[0] > 5 * call
    check(ctx, files["main"], call, tile)


def test_one_piece_of_three_goes_through_a_park(ctx, files):
    from phi_amd.context import TextPark
    park = TextPark(0)
    try:
        check(ctx, files["main"], 5000, 256, park=park)        # the header ends inside a parked piece
        check(ctx, files["small"], 100, 64, park=park)
        hdr = B.parse_header(files["main"])[0]
        check(ctx, files["main"], hdr + 40, 4096, park=park)   # the header and the records of one host piece; then parked ones
        idx = park.add(files["small"])                         # the stream's first piece parked: the header from a fetched prefix
        ctx.reset_reads()
        ctx.reads_bam_begin(1 << 20, 0)
        ctx.add_reads_bam_parked(park, idx)
        got = _records(*ctx.reads_bam_last_batch())
        info = ctx.reads_bam_end()
        assert got == B.decode(files["small"])[0] and info["n_ref"] == 0
    finally:
        park.close()


def _adversarial(fake):
    """A record whose aux `B` array holds a complete, well-formed, plausible chain of six records (fake: else zeros of the same
    size) that begins exactly on a border of the 4 096-byte tiles, and ends in zeros so that it never joins the true chain."""
    rng = np.random.default_rng(3)
    recs, at = [], 0
    for i in range(30):
        r = B.record(b"front%d" % i, _seq(rng, 150), flag=4)
        recs.append(r)
        at += len(r)
    chain = b"".join(B.record(b"fake%d" % i, _seq(rng, 60), flag=4) for i in range(6))
    fixed = 4 + 32 + 8 + 75 + 150 + 8                          # the host record up to the first byte of its aux array
    pad = (-(at + fixed)) % 4096
    assert pad + len(chain) + 64 < 4096 + 4096
    payload = bytes(pad) + (chain if fake else bytes(len(chain))) + bytes(64)
    host = B.record(b"carrier", _seq(rng, 150), flag=4, aux=B.aux_bytes(b"zf", payload))
    fake_at = at + fixed + pad
    assert fake_at % 4096 == 0 and host[fixed + pad:fixed + pad + len(chain)] == (chain if fake else bytes(len(chain)))
    assert (at + len(host)) // 4096 == fake_at // 4096        # the true chain enters the tile the fake chain starts
    recs.append(host)
    for i in range(30):
        recs.append(B.record(b"back%d" % i, _seq(rng, 151), flag=4 | 0x10))
    return B.header() + b"".join(recs)


def test_adversarial_speculation_costs_a_rewalk_and_nothing_else(ctx):
    with_fake, without = _adversarial(True), _adversarial(False)
    assert B.decode(with_fake)[0] == B.decode(without)[0]
    info = check(ctx, with_fake, None, 4096)
    assert info["tiles_rewalked"] >= 1
    info = check(ctx, without, None, 4096)
    assert info["tiles_rewalked"] == 0


def test_reads_of_one_length_reach_the_sketch_without_offsets(ctx):
    rng = np.random.default_rng(9)
    recs = [B.record(b"u%d" % i, _seq(rng, 150), flag=4 | (0x10 if i % 3 == 0 else 0)) for i in range(60)]
    info = check(ctx, B.header() + b"".join(recs), None, 256)
    assert info["one_length"] == 150 and info["batches"] >= 1 and info["batches_without_offsets"] == info["batches"]
    recs[31] = B.record(b"short", _seq(rng, 149), flag=4)
    info = check(ctx, B.header() + b"".join(recs), None, 256)
    assert info["one_length"] == 0 and info["batches"] >= 1 and info["batches_without_offsets"] == 0


# ------------------------------------------------------------------ the same reads as BAM and as FASTQ, on MHC_4
def _hits(ctx):
    import torch
    from phi_amd import dist as pdist
    p, n = ctx.hits_buffer()
    return torch.as_tensor(pdist.DevArray(p, n), device="cuda").cpu().numpy().copy()


def test_bam_equals_its_fastq_on_mhc4(ctx_factory, oracle):
    """A few thousand reads cut from CHM13_reads.fq.gz, a third stored reverse-complemented with 0x10, every seventh cut to
    120 bases: reads_stats, hit vector, spectrum size, solve result and path sequence of the BAM route and the FASTQ route."""
    from phi_amd import ilp_index as H
    g = oracle.parse_gfa(os.path.join(DATA, "MHC_4.gfa.gz"))
    A = g.arrays()
    bases, off, _ = H.read_reads(os.path.join(DATA, "CHM13_reads.fq.gz"))
    raw = bytes(bases)
    reads = [raw[off[i]:off[i + 1]][:120 if i % 7 == 0 else None] for i in range(3000)]
    recs = []
    for i, r in enumerate(reads):
        recs.append(B.record(b"m%d" % i, B.revcomp(r), flag=0x10, ref_id=0, pos=i) if i % 3 == 0 else B.record(b"m%d" % i, r, flag=4))
        if i % 50 == 0:                                        # records that give no read
            recs.append(B.record(b"sup%d" % i, r[:40], flag=0x800, ref_id=0, pos=i))
    bam = B.header(b"@HD\tVN:1.6\n", [(b"chr6", 5_000_000)]) + b"".join(recs)
    got, _ = B.decode(bam)
    assert got == reads
    fq = B.fastq(reads)
    ctx = ctx_factory(k=31, w=25, threshold=1.0, recombination=100)
    ctx.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])

    def outcome():
        st, hits = ctx.reads_stats(), _hits(ctx)
        res = ctx.solve()
        keep = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
        return st, hits, keep, bytes(ctx.path_sequence(res["hap_len"]))

    ctx.reads_bam_begin(1 << 20, 0)
    for i in range(0, len(bam), 300_000):
        ctx.add_reads_bam(bam[i:i + 300_000])
    info = ctx.reads_bam_end()
    assert (info["n_kept"], info["n_reverse"], info["n_secondary_supplementary"]) == (3000, 1000, 60)
    a = outcome()
    ctx.reset_reads()
    ctx.reads_text_begin(1 << 20)
    assert not ctx.add_reads_text(fq)
    pending, taken = ctx.reads_text_end()
    hb, ho = H.reads_of_text(pending, [], stream_offset=taken)
    ctx.add_reads((hb, ho))
    b = outcome()
    assert a[0] == b[0] and a[0]["n_reads"] == 3000
    assert np.array_equal(a[1], b[1]) and a[1].any()
    assert a[2] == b[2] and a[2]["spectrum_size"] > 0
    assert a[3] == b[3] and len(a[3]) > 1000


# ------------------------------------------------------------------ streams the code must refuse by its bounds checks
def _good_prefix(n=5):
    rng = np.random.default_rng(21)
    return B.header(b"@CO\tx\n", [(b"chr1", 1000)]), [B.record(b"ok%d" % i, _seq(rng, 50), flag=0, ref_id=0, pos=i) for i in range(n)]


def _bad_streams():
    hdr, recs = _good_prefix()
    good = hdr + b"".join(recs)
    rng = np.random.default_rng(22)
    out = {"wrong magic": b"BAM\x02" + good[4:], "wrong magic, first byte": b"CRAM" + good[4:],
           "cut inside the header": good[:len(hdr) - 3], "cut inside l_text": good[:6],
           "cut inside a fixed part": good[:len(hdr) + len(recs[0]) + 20],
           "cut inside a sequence": good[:len(hdr) + len(recs[0]) + len(recs[1]) + 36 + 4 + 10]}
    for bs in (-4, 0, 31, 2 ** 31 - 1):
        out["block_size %d" % bs] = good + B.record(b"bad", _seq(rng, 50), flag=0, ref_id=0, block_size=bs) + recs[0]
    out["l_seq -1"] = good + B.record(b"bad", _seq(rng, 50), flag=0, ref_id=0, l_seq=-1) + recs[0]
    out["l_read_name 0"] = good + B.record(b"", b"ACGT", flag=0)[:12] + b"\x00" + B.record(b"", b"ACGT", flag=0)[13:]
    return out


@pytest.mark.parametrize("name", sorted(_bad_streams()))
@pytest.mark.parametrize("call", [None, 50])
def test_invalid_streams_are_refused_with_their_offset(ctx, name, call):
    """PHI_ERR_INVALID with the oracle's byte offset in the detail, from the piece that holds the fault or from the end of the
    stream; what earlier pieces gave stays and nothing of the failing piece is counted; further calls are PHI_ERR_STATE; a
    fresh stream works afterwards."""
    from phi_amd.context import PhiError
    data = _bad_streams()[name]
    with pytest.raises(B.BamInvalid) as oracle_says:
        B.decode(data)
    ctx.reset_reads()
    ctx.reads_bam_begin(1 << 20, 64)
    taken, err, failed_in_add = [], None, False
    step = call or len(data)
    try:
        for i in range(0, len(data), step):
            ctx.add_reads_bam(data[i:i + step])
            taken += _records(*ctx.reads_bam_last_batch())
    except PhiError as e:
        err, failed_in_add = e, True
    if failed_in_add:
        with pytest.raises(PhiError) as again:
            ctx.add_reads_bam(b"\x00" * 40)
        assert again.value.status == STATE
        with pytest.raises(PhiError) as at_end:
            ctx.reads_bam_end()
        assert at_end.value.status == STATE
        info = at_end.value.info
    else:
        with pytest.raises(PhiError) as at_end:
            ctx.reads_bam_end()
        err, info = at_end.value, at_end.value.info
    assert err.status == INVALID, (name, str(err))
    offsets = [int(x) for x in re.findall(r"byte(?: offset)? (\d+)", str(err))]
    assert oracle_says.value.offset in offsets, (name, str(err), oracle_says.value.offset)
    # the whole records in front of the fault, as far as whole pieces held them
    want = B.decode(_good_prefix()[0] + b"".join(_good_prefix()[1]))[0] if not name.startswith(("wrong", "cut inside the header", "cut inside l_text")) else []
    assert taken == want[:len(taken)] and info["n_kept"] == len(taken)
    st = ctx.reads_stats()
    assert st["n_reads"] == len(taken)
    if call is None and failed_in_add:
        assert taken == []                                     # the failing piece was the only one
    # a fresh stream on the same context
    fresh = small_file()
    got, info = run_stream(ctx, fresh, None, 64)
    assert got == B.decode(fresh)[0]


def test_a_record_longer_than_the_buffers_is_unsupported(ctx_factory, oracle, monkeypatch):
    from phi_amd.context import PhiError
    monkeypatch.setenv("PHI_BAM_CARRY", "4096")
    g = oracle.parse_gfa(os.path.join(DATA, "test.gfa"))
    A = g.arrays()
    c = ctx_factory(k=3, w=2, threshold=1.0, recombination=100)
    c.set_graph(A["seq_concat"], A["seq_off"], A["adj_off"], A["adj"], A["walk_off"], A["walk_vtx"], A["top_rank"])
    rng = np.random.default_rng(2)
    data = B.header() + B.record(b"a", _seq(rng, 100), flag=4) + B.record(b"long", _seq(rng, 6000), flag=4)
    c.reads_bam_begin(2048, 64)
    with pytest.raises(PhiError) as e:
        for i in range(0, len(data), 2048):
            c.add_reads_bam(data[i:i + 2048])
    assert e.value.status == -5 and "longer than the stream's buffers" in str(e.value)


def test_bgzf_without_the_end_of_file_block(ctx, files, tmp_path):
    """The writer's BGZF (blocks of 777 inflated bytes, so records straddle them; no empty last block) through the host pool
    that the command line uses, into the stream."""
    from phi_amd import ilp_index as H
    path = str(tmp_path / "x.bam")
    B.write_bam(path, files["main"], block_bytes=777, eof=False)
    assert gzip.decompress(open(path, "rb").read()) == files["main"]
    assert H.reads_file_kind(path) == "bam"
    want, winfo = B.decode(files["main"])
    ctx.reset_reads()
    ctx.reads_bam_begin(1 << 16, 0)
    got = []
    for chunk in H.text_chunks(path, 1 << 16):
        ctx.add_reads_bam(chunk)
        got += _records(*ctx.reads_bam_last_batch())
    info = ctx.reads_bam_end()
    assert got == want and info["n_records"] == winfo["n_records"]
