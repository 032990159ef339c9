"""What `runner.main` refuses from its arguments alone, pinned as a table: for every argv of a fixed grid the first refusal raised (the text of
argparse's `error:` line) or ACCEPTED (the arguments got as far as load_config), compared with tests/golden/cli_refusals.json.  The fixture was
recorded from the main() that preceded `_check_cli`; `python tests/test_cli_refusals_host.py` rewrites it from the code at hand (only to record
a deliberate change of the CLI)."""
import contextlib
import io
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_refusals.json")

TASKS = ("denoising", "super-resolution", "ct", "inpainting")
METHODS = ("mfvi", "dip", "mcd", "sgld")
FLAGS = (("--fits-per-launch", "4"), ("--inpaint-fits", "4"), ("--sibling-fits", "4"), ("--ct-volume", "phantom:2"), ("--predict-samples", "8"),
         ("--calibration",), ("--batch-predict-samples", "4"), ("--batch-calibration",), ("--batch-bookkeeping",), ("--param-dtype", "bf16"),
         ("--sr-downsampler", "lanczos2"), ("--slices-per-launch", "2"), ("--bo-rounds", "1"))
BAD = (("--fits-per-launch", "-1"), ("--inpaint-fits", "-1"), ("--sibling-fits", "-1"), ("--ct-volume", "phantom:0"), ("--ct-volume", "x.npz"),
       ("--predict-samples", "1"), ("--predict-samples", "-2"), ("--batch-predict-samples", "1"), ("--calibration-bins", "0"),
       ("--slices-per-launch", "0"))


def grid():
    """The argument lists behind `--task T --bayes B`, in the order of the fixture's `cases`: task x method x (every subset of up to 3 FLAGS,
    then every subset of up to 1 with each of BAD appended)."""
    subsets = [s for r in range(4) for s in itertools.combinations(FLAGS, r)]
    tails = [sum(s, ()) for s in subsets] + [sum(s, ()) + bad for s in subsets if len(s) <= 1 for bad in BAD]
    return [("--task", t, "--bayes", b) + tail for t in TASKS for b in METHODS for tail in tails]


class _Accepted(Exception):
    pass


def outcomes(save_path):
    """One outcome per case of grid() with load_config and the library both stubbed: "ACCEPTED", or argparse's message from `error:` on with
    the whitespace folded.  Any other exception propagates."""
    from mfvi_dip_mia_amd import _lib, runner

    def accepted(*args, **kw):
        raise _Accepted

    def boom():
        raise AssertionError("the library was loaded")
    saved = runner.load_config, _lib.lib
    runner.load_config, _lib.lib = accepted, boom
    out = []
    try:
        for tail in grid():
            err = io.StringIO()
            try:
                with contextlib.redirect_stderr(err):
                    runner.main(["--config", "unused.json", "--save-path", save_path] + list(tail))
                raise AssertionError("%s: main() returned" % (tail,))
            except _Accepted:
                out.append("ACCEPTED")
            except SystemExit as e:
                text = " ".join(err.getvalue().split())
                assert e.code == 2 and "error:" in text, (tail, e.code, text)
                out.append(text[text.index("error:"):])
    finally:
        runner.load_config, _lib.lib = saved
    return out


def test_cli_refusals_match_the_recorded_table(tmp_path):
    fx = json.load(open(FIXTURE))
    table, cases = fx["outcomes"], fx["cases"]
    got = outcomes(str(tmp_path))
    assert len(got) == len(cases) == 8288
    assert sum(table[c] == "ACCEPTED" for c in cases) == fx["accepted"] == 307      # (a grid that refuses everything would pin nothing)
    assert got.count("ACCEPTED") == fx["accepted"]
    wrong = [(tail, table[c], g) for tail, c, g in zip(grid(), cases, got) if table[c] != g]
    assert not wrong, "%d cases differ, the first: %s\n  recorded: %s\n  now:      %s" % ((len(wrong),) + wrong[0])
    assert sorted(set(got)) == sorted(table) and len(table) == 80
    assert os.listdir(str(tmp_path)) == []                                           # refusing and accepting create no file


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, ROOT)
    with tempfile.TemporaryDirectory() as d:
        got = outcomes(d)
    table = sorted(set(got))
    json.dump(dict(accepted=got.count("ACCEPTED"), outcomes=table, cases=[table.index(g) for g in got]), open(FIXTURE, "w"), separators=(",", ":"))
    print("%d cases, %d distinct outcomes, %d ACCEPTED" % (len(got), len(table), got.count("ACCEPTED")))
