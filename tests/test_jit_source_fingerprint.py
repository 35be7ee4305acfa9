"""Every text the run-time compilation path generates (the translation units of the three kinds of user model, the
closures written out from a descriptor), fingerprinted by a stand-alone host program (tests/cpp/jit_source_fingerprint.cpp)
over a fixed corpus of named cases and compared with tests/golden/jit_source_fingerprints.txt.  A mismatch names the case
that moved; `jit_source_fingerprint --dump DIR` writes the texts, to be diffed against a dump of the commit before.  The
text is the input of the content-keyed code-object cache, so a case that moves compiles every user model of that shape
again on every machine.  The fixture is the output of this program built against the generators as they were moved out of
pmx_jit.cpp, before they were rewritten; regenerate it only for a change that is meant to move the text."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jit_source_fingerprints.txt")


def test_jit_source_fingerprints_match_the_fixture(tmp_path):
    exe = str(tmp_path / "jit_source_fingerprint")
    subprocess.run(["make", "-C", ROOT, "-s", f"JSFPBIN={exe}", "jit_source_fingerprint"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    moved = [f"{w}  ->  {g}" for w, g in zip(want, got) if w != g]
    assert not moved, "texts that moved (fixture -> now):\n" + "\n".join(moved[:40])
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
