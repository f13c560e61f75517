"""DEFLATE that zlib's compressor never writes, through the device inflater (phi_amd.inflate): the streams of
tests/deflate_writer.py at chunk sizes 64 (the floor), 100, 4096 and the default, and once without the finder; every output
byte for byte what zlib's inflater returns.  Then the invalid streams: the status zlib's inflater gives, and the process
goes on.  tests/test_cpu_deflate_writer.py shows, without a GPU, that each stream holds the feature it is named for."""
import gzip
import zlib

import pytest

import deflate_writer as W
from test_cpu_gfa_gzip import split_rule

pytestmark = pytest.mark.gpu

RUNS = [(64, True), (100, True), (4096, True), (0, True), (4096, False)]


@pytest.fixture(scope="module")
def phi():
    import __graft_entry__
    __graft_entry__.ensure_built()
    import phi_amd
    return phi_amd


@pytest.fixture(scope="module")
def want():
    """{name: what zlib's inflater returns} (the reference: computed once)"""
    return {name: gzip.decompress(s.data) for name, s in W.valid_streams().items()}


@pytest.mark.parametrize("chunk,finder", RUNS, ids=["c64", "c100", "c4096", "default", "c4096_no_finder"])
@pytest.mark.parametrize("name", W.VALID)
def test_stream_matches_zlib(phi, want, name, chunk, finder):
    s = W.valid_streams()[name]
    out, info = phi.inflate(s.data, chunk_bytes=chunk, finder=finder)
    assert len(out) == len(want[name]) and out == want[name], (name, chunk, finder, len(out), len(want[name]))
    assert info["out_bytes"] == len(want[name]) and info["members"] == s.members
    if finder and chunk in s.aligned:
        # the block the family is about opens a piece of its own: what it copies from before itself went through markers
        assert info["confirmed"] >= 1 and info["marker_bytes"] > 0, info
    if not finder:
        assert info["confirmed"] == 0 and info["marker_bytes"] == 0


def test_small_blocks_through_the_park_and_the_gfa_split(phi, want, ctx_factory):
    """TextPark.add_gzip and phi_gfa_gzip_split inflate through the same decoder (phi_inflate_to_device): family E, whose
    text is a GFA, through both"""
    s, text = W.valid_streams()["E_small_blocks"], want["E_small_blocks"]
    park = phi.TextPark(0)
    piece = 64 << 10
    idx, info = park.add_gzip([s.data[:1], s.data[1:100_001], s.data[100_001:]], piece)
    assert b"".join(park.fetch(i) for i in idx) == text and len(idx) == -(-len(text) // piece)
    assert info["out_bytes"] == len(text) and info["members"] == 1
    park.close()
    want_host, walks = split_rule(text)
    ctx = ctx_factory(k=3, w=2, threshold=1.0, recombination=100)
    for chunk in (64, 0):
        host, ginfo = ctx.gfa_gzip_split(s.data, chunk)
        assert host == want_host
        assert ginfo["text_bytes"] == len(text) and ginfo["n_walks"] == len(walks) > 1000
        assert ginfo["walk_bytes"] == sum(e - b for b, e in walks) and ginfo["inflate"]["out_bytes"] == len(text)


@pytest.mark.parametrize("name", list(W.INVALID))
def test_invalid_stream_is_refused_as_zlib_refuses_it(phi, name):
    from phi_amd import PHI_ERR_INVALID, PhiError
    data = W.invalid_stream(name)
    with pytest.raises(zlib.error, match=W.INVALID[name][1]):
        zlib.decompressobj(31).decompress(data)
    for chunk in (64, 4096, 0):
        with pytest.raises(PhiError) as e:
            phi.inflate(data, chunk_bytes=chunk)
        assert e.value.status == PHI_ERR_INVALID, (name, chunk, e.value)
    good = W.valid_streams()["H_phases"]
    assert phi.inflate(good.data, chunk_bytes=64)[0] == gzip.decompress(good.data)
