"""The prefix sums of phi_amd/csrc/scan.hip at their own borders (phi_prefix_sums): 1024 items per workgroup of the three
phases, 4096 per turn of the single workgroup, the switch between the two at 8192 items, and more than 4096 block sums (two
turns of the single workgroup over them).  Every kind against numpy.cumsum with a leading zero, computed in int64 and cast;
the output starts out as 0xC0 bytes and holds one item more than the scan may write.

Run as `python tests/test_gpu_scan.py reuse` it is the child of test_scratch_reuse_with_everything_pooled."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 1024 * 1024, 4096 * 1024 + 5]
IN_DTYPE = {0: np.uint8, 1: np.int32, 2: np.int32}
OUT_DTYPE = {0: np.int32, 1: np.int32, 2: np.int64}
GUARD = 0xC0
_CASES = {}


def _case(kind, n, fill="random"):
    """(input, expected n + 1 sums), made once and never written to"""
    key = (kind, n, fill)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * kind + n % 977)
        if fill == "zeros":
            x = np.zeros(n, IN_DTYPE[kind])
        elif fill == "ones":
            x = np.ones(n, IN_DTYPE[kind])
        else:
            # kind 1: totals up to 255 * (4096 * 1024 + 5) < 2^31; kind 2: past 2^32 from four items on
            high = {0: 256, 1: 256, 2: 1 << 30}[kind]
            x = rng.integers(0, high, size=n, dtype=np.int64).astype(IN_DTYPE[kind])
        want = np.concatenate([np.zeros(1, np.int64), np.cumsum(x.astype(np.int64))])
        if kind != 2:
            assert want[-1] < (1 << 31)
        x.setflags(write=False)
        want = want.astype(OUT_DTYPE[kind])
        want.setflags(write=False)
        _CASES[key] = (x, want)
    return _CASES[key]


def _run(ctx, kind, n, fill="random", in_place=False):
    import torch
    x, want = _case(kind, n, fill)
    isz = np.dtype(OUT_DTYPE[kind]).itemsize
    out = torch.full(((n + 2) * isz,), GUARD, dtype=torch.uint8, device="cuda")
    if in_place:
        assert kind == 1
        out[:n * 4] = torch.from_numpy(x.view(np.uint8).copy()).cuda()
        d_in = out.data_ptr()
    else:
        src = torch.from_numpy(x.copy()).cuda() if n else torch.zeros(1, dtype=torch.uint8, device="cuda")
        d_in = src.data_ptr()
    torch.cuda.synchronize()
    ctx.prefix_sums(kind, d_in, n, out.data_ptr())
    got = out.cpu().numpy()
    sums = got[:(n + 1) * isz].view(OUT_DTYPE[kind])
    bad = np.flatnonzero(sums != want)
    assert bad.size == 0, (kind, n, fill, in_place, bad[:4].tolist(), sums[bad[:4]].tolist(), want[bad[:4]].tolist())
    assert (got[(n + 1) * isz:] == GUARD).all(), (kind, n, "written past n + 1 items")


@pytest.fixture(scope="module")
def ctx(ctx_factory):
    return ctx_factory()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_prefix_sums(ctx, kind, n):
    _run(ctx, kind, n)


@pytest.mark.parametrize("n", SIZES)
def test_prefix_sums_in_place(ctx, n):
    _run(ctx, 1, n, in_place=True)


@pytest.mark.parametrize("fill", ["zeros", "ones"])
def test_wide_sums_of_zeros_and_ones(ctx, fill):
    _run(ctx, 2, SIZES[-1], fill)


def _large_small_large(ctx):
    """scratch that grows, is reused by a smaller scan and by a larger one again: no sum depends on what it held"""
    for n in (1025, SIZES[-1], 5, 8193, SIZES[-1], 1024 * 1024):
        for kind in (0, 1, 2):
            _run(ctx, kind, n)
        _run(ctx, 1, n, in_place=True)


def test_scratch_reuse_on_one_context(ctx_factory):
    _large_small_large(ctx_factory())


def test_scratch_reuse_with_everything_pooled():
    """the same in a child whose pool keeps every buffer that is let go (PHI_DEVICE_POOL_MIN=0), as test_gpu_dirty_memory.py
    runs its battery"""
    env = {k: v for k, v in os.environ.items() if k not in ("PHI_DEVICE_POISON", "PHI_DEVICE_POOL_MIN", "PHI_DEVICE_POOL")}
    env["PHI_DEVICE_POOL_MIN"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "reuse"], capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("reuse ok"), (r.returncode, (r.stdout[-300:] + r.stderr)[-3000:])


def test_refusals_launch_nothing(ctx):
    import torch
    import phi_amd
    src = torch.ones(16, dtype=torch.int32, device="cuda")
    out = torch.full((17 * 8,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for kind, d_in, n, d_out in ((1, src.data_ptr(), -1, out.data_ptr()), (3, src.data_ptr(), 16, out.data_ptr()),
                                 (-1, src.data_ptr(), 16, out.data_ptr()), (2, 0, 16, out.data_ptr()), (0, src.data_ptr(), 16, 0),
                                 (1, 0, 0, 0)):
        with pytest.raises(phi_amd.PhiError) as e:
            ctx.prefix_sums(kind, d_in, n, d_out)
        assert e.value.status == phi_amd.PHI_ERR_INVALID, (kind, n)
    ctx.device_synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    _run(ctx, 1, 5)                                   # and the context goes on working


if __name__ == "__main__":
    assert sys.argv[1:] == ["reuse"]
    import __graft_entry__
    __graft_entry__.ensure_built()
    import phi_amd
    c = phi_amd.Context(0)
    _large_small_large(c)
    c.close()
    print("reuse ok")
