"""No result may depend on what device memory held before.  Every kernel test of the suite starts from a fresh context on
memory the driver has cleared; in real use a buffer comes back from the pool of dev_mem.hip with an earlier owner's contents, or
stays with its context from a larger input to a smaller one.  Here the battery of tests/dirty_battery.py -- the smallest shapes
that still reach every kernel family, each case asserted against its CPU reference inside the child -- runs

    clean     no variable set: the baseline digest, once per group
    pooled    PHI_DEVICE_POOL_MIN=256: every buffer that is let go is kept for the next taker, contents and all
    ff        PHI_DEVICE_POISON=0xff: every buffer starts out as -1 / NaN / all flags set (and maybe as an "empty" sentinel,
              which is why one byte is not enough)
    80        ... as large negative 32-bit values (the kind NEGK + x wraps on)
    7f        ... as large positive values
    01        ... as small non-zero counters

and passes when the child's exit status is 0 (every case equals its CPU reference) and its digest -- integers and hashes of
arrays, no time, no address, no tolerance -- equals the clean one exactly.  The group `reuse` is about buffers a context keeps:
input B after a different input A on one context, against B on a fresh one.

One child at a time.  A child that ends on a signal, with status 134 or 139, at its time limit or with a HIP illegal-access
error is recorded, and every later test of the module fails at once WITHOUT starting a child: nothing more goes to the GPU
after a fault.  Correct code never reads memory it has not written and runs this mode without a fault; one met here is a
finding, to be understood from the code.

Wall time of one child on clean memory, MI355X, interpreter start and context creation included (seconds):
    reads 2.5   solve 2.7   text 2.5   graphs 2.3   vcf 3.2   edit 3.5   ladder 2.3   reuse 3.0
(the dirty variants: 2.2 .. 4.0; the whole module, 48 children: 134 s)
(the golden VCF is a group of its own: with the chop and class-table cases in one child the group went over five seconds)"""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

import dirty_battery

pytestmark = pytest.mark.gpu

GROUPS = list(dirty_battery.GROUPS)
VARIANTS = {
    "pooled": {"PHI_DEVICE_POOL_MIN": "256"},
    "ff": {"PHI_DEVICE_POISON": "255"},
    "80": {"PHI_DEVICE_POISON": "128"},
    "7f": {"PHI_DEVICE_POISON": "127"},
    "01": {"PHI_DEVICE_POISON": "1"},
}
SECONDS = 5                                       # what a child may take; its time limit is sized as test_gpu_fuzz.py sizes its own
FAULTS = []                                       # the first child that faulted, hung or aborted: nothing runs after it


def _run_child(group, variant):
    if FAULTS:
        pytest.fail(f"not started: an earlier child faulted ({FAULTS[0]})")
    env = {k: v for k, v in os.environ.items() if k not in ("PHI_DEVICE_POISON", "PHI_DEVICE_POOL_MIN", "PHI_DEVICE_POOL")}
    env.update(VARIANTS.get(variant, {}))
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dirty_battery.py"), group], capture_output=True, text=True,
                           timeout=SECONDS + 240, cwd=ROOT, env=env)
    except subprocess.TimeoutExpired as e:
        FAULTS.append(f"{group}/{variant}: no end after {e.timeout} s")
        pytest.fail(FAULTS[0])
    wall = time.perf_counter() - t0
    tail = (r.stdout[-300:] + r.stderr)[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stdout + r.stderr:
        FAULTS.append(f"{group}/{variant}: exit status {r.returncode}")
        pytest.fail(FAULTS[0] + "\n" + tail)
    print(f"dirty_battery {group}/{variant}: {wall:.1f} s")
    assert r.returncode == 0, tail
    digest = json.loads(r.stdout.strip().splitlines()[-1])
    assert digest and all(digest.values()), digest
    return digest


@pytest.fixture(scope="module")
def clean(oracle):
    """group -> the digest of the battery on clean memory, computed once"""
    import __graft_entry__
    __graft_entry__.ensure_built()
    seen = {}

    def get(group):
        if group not in seen:
            seen[group] = None                    # (a baseline that failed is not tried again for every variant)
            seen[group] = _run_child(group, "clean")
        if seen[group] is None:
            pytest.fail(f"the clean run of {group} failed")
        return seen[group]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("group", GROUPS)
def test_dirty_memory_changes_nothing(clean, group, variant):
    want = clean(group)
    got = _run_child(group, variant)
    assert got.keys() == want.keys()
    diff = {c: {k: (got[c].get(k), want[c].get(k)) for k in set(got[c]) | set(want[c]) if got[c].get(k) != want[c].get(k)} for c in want}
    diff = {c: d for c, d in diff.items() if d}
    assert not diff, diff
