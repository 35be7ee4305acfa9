"""Everything the population compiler produces (op stream, class plan, step, op and program records, chunk headers),
fingerprinted field by field by a stand-alone host program (tests/cpp/plan_fingerprint.cpp) over a fixed corpus of
(population, CompileKey) cases and compared with tests/golden/plan_fingerprints.txt.  A mismatch names the case and
the array that moved.  The fixture is the output of this program built against the host compiler sources of the
commit before pmx_plan.cpp was split off; regenerate it only for a change that is meant to move a layout.  Moved since, on
purpose: ragged_g4_min1 and edges_g4_min1 (classes of one member allowed), 23 lines each, when build_class_plan began to
leave subjects that never propagate to the generic walker; the other 55 cases are as recorded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_fingerprints.txt")


def test_plan_fingerprints_match_the_fixture(tmp_path):
    exe = str(tmp_path / "plan_fingerprint")
    subprocess.run(["make", "-C", ROOT, "-s", f"FPBIN={exe}", "plan_fingerprint"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    moved = [f"{w}  ->  {g}" for w, g in zip(want, got) if w != g]
    assert not moved, "fields that moved (fixture -> now):\n" + "\n".join(moved[:40])
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
