"""The hand-written DEFLATE streams of tests/deflate_writer.py, checked without a GPU: zlib's inflater accepts every valid
one and returns the text the writer followed, the walker finds in each the feature it is named for, and zlib's inflater
refuses every invalid one for the reason it is named for.  tests/test_gpu_deflate_shapes.py runs the same streams through
the device inflater; this module is what keeps a stream there from having lost its point."""
import gzip
import zlib

import pytest

import deflate_writer as W


@pytest.fixture(scope="module")
def walked():
    """{name: (stream, the walker's stats, per member (end phase, output bytes, last block's output bytes))}"""
    out = {}
    for name, s in W.valid_streams().items():
        text, st, ends = W.walk_gzip(s.data)
        assert text == s.text, name
        out[name] = (s, st, ends)
    return out


def test_the_tables_are_those_of_rfc_1951():
    assert W.LBASE == [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    assert W.DBASE == [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                       4097, 6145, 8193, 12289, 16385, 24577]
    assert len(W.LEXT) == 29 and len(W.DEXT) == 30 and max(W.LEXT) == 5 and max(W.DEXT) == 13


def test_the_walker_reads_what_zlib_writes():
    text = W.fastq_like(200_000, 3)
    for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        raw = c.compress(text) + c.flush()
        out, st, end = W.walk(raw)
        assert out == text and (end + 7) // 8 == len(raw)
        assert st["max_distance"] <= 32768 - 262 and st["one_code_dist_trees"] == st["zero_code_dist_trees"] == 0


@pytest.mark.parametrize("name", W.VALID)
def test_zlib_accepts_and_returns_the_text(name):
    s = W.valid_streams()[name]
    assert len(s.text) <= 1 << 20 and len(s.data) <= 300_000
    if s.members == 1:
        d = zlib.decompressobj(31)
        assert d.decompress(s.data) == s.text and d.eof and not d.unused_data
    else:
        assert gzip.decompress(s.data) == s.text
        assert s.data.count(b"\x1f\x8b\x08") >= s.members


def _aligned_blocks(s, st):
    return [at for at, _, _ in st["starts"] if all(at % (8 * a) == 0 for a in s.aligned)]


def test_a_far_distances(walked):
    far = {W.dist_symbol(d) for d in W.FAR}
    for name in ("A_far", "A_far_aligned"):
        s, st, _ = walked[name]
        assert st["max_distance"] == 32768 and far <= st["dist_pairs"] and {(257, 0), (285, 0)} <= st["len_pairs"]
    s, st, _ = walked["A_far_aligned"]
    at = st["starts"][1][0]
    assert s.aligned == (64, 100, 4096) and at in _aligned_blocks(s, st) and st["starts"][1][1:] == (2, 0)
    assert (at, 32768, 3) in st["first_matches"]                              # marker 256 opens the piece
    assert s.text[32768 + 3:32768 + 3 + 4] == s.text[32767:32768] + s.text[:3]   # then the byte before it: 256 + 32767
    s, st, _ = walked["A_member_start"]
    assert s.members == 2 and st["matches_to_first_byte"] == 2
    at = st["starts"][-2][0]
    assert at in _aligned_blocks(s, st) and (at, 1040, 258) in st["first_matches"]


def test_b_trees_zlib_never_writes(walked):
    _, st, _ = walked["B_trees"]
    assert st["zero_code_dist_trees"] >= 4 and st["one_code_dist_trees_used"] >= 3
    assert st["one_code_lit_trees"] == 1 and (2, 0) in st["empty"]
    assert {(257, 1), (286, 30), (265, 5), (276, 4)} <= st["shapes"] and 11 in {hdist for _, hdist in st["shapes"]}
    assert min(st["hclen"]) == 5 and 19 in st["hclen"]
    assert st["max_cl_bits"] == 7
    for before in (17, 18):
        assert any(sym == 16 and b == before and i < hlit < i + rep for sym, rep, i, hlit, b in st["cl_events"]), before
    assert any(sym == 18 and rep == 138 for sym, rep, *_ in st["cl_events"])
    assert st["max_lit_bits"] == 15 and st["max_dist_bits"] == 15 and st["all_ones_15"] == {"lit", "dist"}
    assert st["long_lit_symbols"] > 500 and st["long_dist_symbols"] > 20
    assert (285, 0) in st["len_pairs"] and (29, 8191) in st["dist_pairs"]


def test_c_every_base_and_extra(walked):
    _, st, _ = walked["C_sweep"]
    assert st["matches"] == 3480 and (284, 31) in st["len_pairs"] and (285, 0) in st["len_pairs"]
    assert st["len_pairs"] == {(257 + i, x) for i in range(29) for x in (0, (1 << W.LEXT[i]) - 1)}
    assert st["dist_pairs"] == {(i, x) for i in range(30) for x in (0, (1 << W.DEXT[i]) - 1)}
    assert st["max_distance"] == 32768


def test_d_overlapping_copies(walked):
    want = {(d, n) for d in range(1, 67) for n in W.OVERLAP_LENGTHS if d < n}
    assert len(want) == 2 + 62 + 63 + 64 + 65 + 5 * 66                       # (lengths 3, 63, 64, 65, 66; the longer ones always)
    for name in ("D_overlap", "D_overlap_aligned"):
        assert want <= walked[name][1]["overlaps"], name
    s, st, _ = walked["D_overlap_aligned"]
    dyn = [at for at, t, _ in st["starts"] if t == 2]
    assert len(dyn) == 660 and all(at % (64 * 8) == 0 for at in dyn)
    assert len(st["first_matches"]) == 330 + 5                               # the others begin with distance // 2 literals


def test_e_many_small_blocks(walked):
    _, st, _ = walked["E_small_blocks"]
    assert sum(st["blocks"].values()) >= 19_000 and min(st["blocks"].values()) >= 3000
    assert st["min_block_out"] == 0 and st["max_block_out"] <= 40
    assert st["blocks_reached"] >= 20_000 and st["max_distance"] > 32_000
    assert {(at % 8, t) for at, t, _ in st["starts"]} >= {(p, t) for p in range(8) for t in (1, 2)}
    assert st["one_code_dist_trees_used"] > 100 and st["zero_code_dist_trees"] > 100
    assert (0, 0) in st["empty"] and (1, 0) in st["empty"] and (2, 0) in st["empty"]


def test_f_empty_blocks_and_fixed_runs(walked):
    for name, kind in (("F_final_empty_stored", 0), ("F_final_empty_fixed", 1), ("F_final_empty_dynamic", 2)):
        _, st, _ = walked[name]
        assert st["empty"] == {(0, 0), (1, 0), (2, 0), (kind, 1)} and st["final_type"] == kind, name
    _, st, _ = walked["F_final_stored"]
    assert st["final_type"] == 0 and st["last_block_out"] > 0 and st["empty"] == {(0, 0), (1, 0), (2, 0)}
    _, st, _ = walked["F_fixed_run"]
    run = [at for at, t, f in st["starts"][1:-1] if t == 1 and not f]
    assert len(run) == 300 == len(st["starts"]) - 2 and run[-1] - run[0] > 8 * 5 * 4096


def test_g_decoys():
    s, payload = W.family_g_decoy_deflate()
    assert payload in s.data and payload in s.text and 50_000 < len(payload) <= 65535
    out, st, end = W.walk(payload)
    assert out == zlib.decompress(payload, -15) and (end + 7) // 8 == len(payload)
    assert st["blocks"][2] > 100                                             # each a start that decodes cleanly
    s, payload = W.family_g_decoy_gzip()
    assert payload in s.data and payload in s.text and payload[7:10] == b"\x1f\x8b\x08"
    assert gzip.decompress(payload[7:]) == W.fastq_like(60_000, 72)


def test_h_members(walked):
    s, st, ends = walked["H_members"]
    full = [e for e in ends if e[1]]
    assert len(ends) == s.members == 39 and len(full) == 20 and all(last == 10 for _, _, last in full)
    s, st, ends = walked["H_phases"]
    assert [phase for phase, _, _ in ends] == [i % 8 for i in range(16)]


def test_what_the_new_streams_hold(walked, capsys):
    """the figures DESIGN.md 4.8 states for the new streams (those of the zlib matrix were 32 505 and no such tree)"""
    top = max(st["max_distance"] for _, st, _ in walked.values())
    one = sum(st["one_code_dist_trees"] for _, st, _ in walked.values())
    used = sum(st["one_code_dist_trees_used"] for _, st, _ in walked.values())
    zero = sum(st["zero_code_dist_trees"] for _, st, _ in walked.values())
    with capsys.disabled():
        print("\nnew streams: largest distance %d, one-code distance trees %d (%d used by a match), zero-code %d" % (top, one, used, zero))
    assert top == 32768 and used > 0 and zero > 0


@pytest.mark.parametrize("name", list(W.INVALID))
def test_zlib_refuses_for_the_reason_named(name):
    data = W.invalid_stream(name)
    d, got = zlib.decompressobj(31), b""
    with pytest.raises(zlib.error, match=W.INVALID[name][1]):
        for i in range(len(data)):
            got += d.decompress(data[i:i + 1])
    assert got.startswith(W.INVALID_PREFIX)                     # good up to the block that is spoilt
    with pytest.raises(Exception):
        gzip.decompress(data)
