"""Host-inclusive cost of Tracking::SearchLocalPoints' second loop and matcher call (reference src/Tracking.cc:1433-1463) through the
compiled adaptors (tests/adapter_localmap_driver.cc `bench`, built WITHOUT the capture hook), the adaptor's own work inside the clock:
  (a) the parent route: Frame::isInFrustum per point on the host, then the resident map-point search (adapter/ORBmatcher_proj.cc)
  (b) orbx_adapter::SearchLocalPoints, one orbx_frame_search_local_points call, nothing changed in the resident table
  (c) the same after 5 % of the points changed geometry (they are re-sent in the one orbx_mappoints_set in front of the search)
at 2 000 and 8 000 local points x 1 000 features; medians of --reps rounds in which the three alternate.  With --trace the bench runs once
more under rocprofv3 --kernel-trace --stats (a run of its own: its timings are not reported) for k_frustum's line.
Run on the GPU box: python tools/bench_local_points.py [--out FILE] [--reps 200] [--trace]"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge                    # noqa: E402
import test_local_points_adapter as TA          # noqa: E402

SIZES = ((2000, 1000), (8000, 1000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    pkg = ge.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# SearchLocalPoints, second loop + search, adaptor-inclusive (std::chrono in the compiled driver), medians of {a.reps} rounds in "
        f"microseconds; device: {pkg.orbx.device_identity(0)}")
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        exe = TA.build_driver(tmp, capture=False)
        for npts, nfeat in SIZES:
            run = subprocess.run([exe, "bench", str(npts), str(nfeat), str(a.reps)], capture_output=True, text=True, timeout=300)
            if run.returncode != 0:
                say(f"{npts} points: bench FAILED: {run.stderr.strip()}")
                return 1
            t = {}
            for ln in run.stdout.splitlines():
                f = ln.split()
                if f[0].startswith("time_"):
                    t[f[0][5:]] = int(f[1]) / 1000.0
                else:
                    head = ln
            say(f"{npts} local points x {nfeat} features ({head})")
            say(f"  (a) host isInFrustum loop + resident search      {t['a']:8.1f}")
            say(f"  (b) one call, table unchanged                    {t['b']:8.1f}   ({t['a'] / t['b']:.2f}x)")
            say(f"  (c) one call, 5 % of the points re-sent          {t['c']:8.1f}   ({t['a'] / t['c']:.2f}x)")
            ok = ok and t["b"] < t["a"]
        say(f"(b) below (a) at both sizes: {'yes' if ok else 'NO'}")
        if a.trace:
            out = os.path.join(tmp, "trace")
            run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", exe, "bench", "8000", "1000", "50"],
                                 capture_output=True, text=True, timeout=300)
            found = False
            for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if any(k in row.get("Name", "") for k in ("k_frustum", "k_proj_lists", "k_proj_resolve", "k_mappoints_scatter")):
                        say(f"  kernel {row['Name'].split('(')[0]:24s} calls {row.get('Calls')}   average {float(row.get('AverageNs', 'nan')) / 1000.0:7.2f} us   "
                            f"min {float(row.get('MinNs', 'nan')) / 1000.0:7.2f}   max {float(row.get('MaxNs', 'nan')) / 1000.0:7.2f}   "
                            f"(8000 points x 1000 features, under the profiler)")
                        found = True
            if not found:
                say("  kernel trace: no stats file found: " + run.stderr.strip()[-300:])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
