#!/usr/bin/env python3
"""The GFA stage from a .gfa.gz, host against device: the native generator's graph of a configuration (C2: 49
walks x 5 Mbp, 77 MB of text; C5: 200 walks x 170 Mbp, 10.9 GB) written to a RAM disk and compressed as ONE gzip member by
16 host threads (pigz-style: profiles/c5_files.py gzip_file), then, alternating, --runs times each:
  host    the command line's PHI_GFA_INFLATE=0 path: phi_gfa_read_deferred on the file (zlib on one thread), walks resolved
          on the device when their text is at least PHI_WALK_TEXT_MIN (1 GB), else on the host
  device  DeferredGraph.from_gzip_on_device: read the file, phi_gfa_gzip_split, phi_gfa_read_deferred_text, walks resolved
          on the device from the fields that never left it
Each leg runs in a fresh process (the timings include nothing of the other leg's state).  Kernel times: run the device leg
alone under `rocprofv3 --kernel-trace --stats` (--legs device --runs 1 --reuse).

    python3 profiles/gfa_gzip_rate.py [--configs C2,C5] [--runs 3] [--dir /dev/shm/phi_gfagz] [--keep | --reuse] [--out f.json]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def leg(kind, path):
    """one GFA stage in this process: seconds and what it found"""
    import resource
    import phi_amd
    from phi_amd import ilp_index as H
    ctx = phi_amd.Context(0)                       # (the device starts before the clock, in both legs)
    t0 = time.perf_counter()
    if kind == "device":
        g = H.DeferredGraph.from_gzip_on_device(path, ctx)
        route, info = g.route, g.split_info
    else:
        g = H.DeferredGraph(path)
        walk_bytes = sum(n for _, n in g.walk_texts())
        route = "host"
        if not (walk_bytes >= (1 << 30) and g.resolve_on_device(ctx)):
            g.resolve_on_host()
        info = {"walk_bytes": walk_bytes}
    dt = time.perf_counter() - t0
    out = {"leg": kind, "route": route, "gfa_stage_s": round(dt, 4), "n_walks": g.num_walks, "n_vtx": g.n_vtx,
           "walks_on_device": g.on_device, "max_rss_gb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20, 3)}
    if kind == "device":
        out.update({k: info[k] for k in ("text_bytes", "host_bytes", "walk_bytes")})
        out["inflate_device_ms"] = round(info["inflate"]["device_ms"], 2)
        out["gzip_bytes"], out["chunks"] = info["inflate"]["in_bytes"], info["inflate"]["chunks"]
    g.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C5")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--legs", default="device,host")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--dir", default="/dev/shm/phi_gfagz")
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--reuse", action="store_true", help="the .gfa.gz of an earlier --keep run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", nargs=2, help=argparse.SUPPRESS)        # (the child process of one leg)
    args = ap.parse_args()
    if args.leg:
        return leg(*args.leg)
    from phi_amd import synth
    from c5_files import gzip_file
    os.makedirs(args.dir, exist_ok=True)
    res = {"level": args.level, "configs": {}}
    try:
        for cfg in args.configs.split(","):
            gz = os.path.join(args.dir, cfg + ".gfa.gz")
            rec = {}
            if not (args.reuse and os.path.exists(gz)):
                gk = synth.NATIVE_CONFIGS[cfg][0] if cfg in synth.NATIVE_CONFIGS else synth.CONFIGS[cfg][0]
                plain = os.path.join(args.dir, cfg + ".gfa")
                g = synth.NativeGraph(**gk)
                rec["gfa_bytes"] = g.write_gfa(plain)
                g.close()
                t0 = time.perf_counter()
                rec["gz_bytes"] = gzip_file(plain, gz, args.level)
                rec["compress_s"] = round(time.perf_counter() - t0, 2)
                os.remove(plain)
            runs = []
            for i in range(args.runs):
                for kind in args.legs.split(","):
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, gz], capture_output=True, text=True, timeout=900)
                    if r.returncode != 0:
                        print(r.stderr[-3000:], flush=True)
                        raise SystemExit(f"{cfg} {kind}: exit status {r.returncode}")
                    runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
                    print(cfg, json.dumps(runs[-1]), flush=True)
            rec["runs"] = runs
            for kind in args.legs.split(","):
                xs = sorted(x["gfa_stage_s"] for x in runs if x["leg"] == kind)
                if xs:
                    rec[kind + "_median_s"] = xs[len(xs) // 2]
            if "device_median_s" in rec and "host_median_s" in rec:
                rec["host_over_device"] = round(rec["host_median_s"] / rec["device_median_s"], 2)
            res["configs"][cfg] = rec
    finally:
        if not args.keep:
            shutil.rmtree(args.dir, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({c: {k: v for k, v in r.items() if k != "runs"} for c, r in res["configs"].items()}))


if __name__ == "__main__":
    main()
