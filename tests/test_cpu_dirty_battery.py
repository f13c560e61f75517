"""tests/dirty_battery.py where no GPU is present: every case of every group builds its input and passes its own CPU
reference (--reference-only), every group has cases, and nothing a digest holds is a time."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

import dirty_battery


def test_every_group_has_cases_and_the_issue_names_them():
    assert set(dirty_battery.GROUPS) >= {"reads", "solve", "text", "graphs", "edit", "ladder", "reuse"}
    for group, cases in dirty_battery.GROUPS.items():
        assert cases, group
        assert len({name for name, _ in cases}) == len(cases)


def test_reference_only_passes_for_every_group(oracle):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dirty_battery.py"), "all", "--reference-only"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    digest = json.loads(r.stdout.strip().splitlines()[-1])
    want = {f"{g}.{name}" for g, cases in dirty_battery.GROUPS.items() for name, _ in cases}
    assert set(digest) == want
    assert "libphi_amd" not in r.stderr


def test_a_digest_holds_no_time_and_no_float():
    d = dirty_battery.D(dict(objective=7, expand_gpu_ms=0.25, read_s=1.5, mean_classes=3.2, path=np.arange(4, dtype=np.int32),
                             stats=dict(n=3, walks_gpu_ms=1.0), text=b"ACGT"))
    assert set(d) == {"objective", "path", "stats.n", "text"} and d["objective"] == 7 and d["stats.n"] == 3
    assert not any(k.endswith("_ms") for k in dirty_battery.flat(dict(a=d)))
    assert dirty_battery.H(np.arange(4, dtype=np.int32)) != dirty_battery.H(np.arange(4, dtype=np.int64))
    assert dirty_battery.H([b"AC", b"GT"]) != dirty_battery.H([b"A", b"CGT"])
