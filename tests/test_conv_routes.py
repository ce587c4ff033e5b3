"""The convolution dispatch of csrc/igemm.hip, seen through its query entry points (no GPU): which tile each direction runs, whether
the input transform is fused, the BatchNorm-statistics split count and the workspace size, for every geometry of the committed
tile table and of the GPU kernel tests, under each GEMM arithmetic and under a sweep of pinned tiles.  The expected values
(tests/golden/conv_routes.json) were recorded with tools/record_conv_routes.py BEFORE the route functions replaced the in-line
re-planning of the entry points: a difference is a changed routing decision."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDER = os.path.join(ROOT, "tools", "record_conv_routes.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_routes.json")


def test_dispatch_matches_the_recorded_routes():
    # a fresh process without CSTP_* variables: dispatch reads several once per process and keeps tiles in a process-wide map
    env = {k: v for k, v in os.environ.items() if not k.startswith("CSTP_")}
    r = subprocess.run([sys.executable, RECORDER, "--rows"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout)
    with open(FIXTURE) as f:
        want = json.load(f)
    assert len(want["tuned"]) >= 3 * 56 and sorted(want["tuned"]) == sorted(want["sweep"])
    bad = []
    for sec in ("tuned", "sweep"):
        for name in sorted(set(want[sec]) | set(got[sec])):
            w, g = want[sec].get(name), got[sec].get(name)
            if w == g:
                continue
            bad.append((sec, name))
            if sec == "tuned":
                print("tuned %s\n  recorded %s\n  now      %s" % (name, json.dumps(w), json.dumps(g)))
            else:       # the fixture keeps a digest of a geometry's sweep: print the rows that no longer hash to it
                print("sweep %s: digest %s != recorded %s; its rows now:" % (name, g, w))
                for row in got["sweep_rows"].get(name, []):
                    print("  " + json.dumps(row))
    assert not bad, "%d routing records differ from tests/golden/conv_routes.json (rows above): %s" % (len(bad), bad[:8])
