"""The drop-in boundary, pinned by the REFERENCE's own command line (src/smudgeplot/cli.py:18-72, 348-382).

tests/golden/cli_argv.json holds the argument vectors the reference command line hands its executables, recorded from the
reference's own code (tests/golden/make_cli_argv.py), for the documented grammar and for the literal command lines below.
* On a machine without a GPU: the command line (smudgeplot_amd/cli.py, which resolves and runs the executables the way
  the reference's get_binary_path / run_binary do) is run with smudgeplot_amd/bin first on PATH.  It must call OUR
  executables with exactly the reference's argument vectors, and surface our exit status the way the reference surfaces
  its binary's: the run gets as far as the engine's "no HIP device" (there is no CPU fallback).
* On the GPU: the recorded argument vectors are replayed against the drop-in executables and the `.smu` / smudge files
  are compared with the golden vectors made by the reference binaries."""
import json
import os
import shlex
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_golden
from smudgeplot_amd import ktab

BIN = os.path.join(ROOT, "smudgeplot_amd", "bin")
ARGV = json.load(open(os.path.join(GOLDEN, "cli_argv.json")))


def _cli(case, cwd):
    """the recorded reference command line `case` through the drop-in's command line, the executables first on PATH"""
    env = dict(os.environ, PATH=BIN + os.pathsep + os.environ.get("PATH", ""), PYTHONPATH=ROOT, MPLBACKEND="Agg")
    return subprocess.run([sys.executable, "-m", "smudgeplot_amd", *ARGV[case]["cli"]], cwd=cwd, capture_output=True, text=True,
                          env=env)


def _calling(case):
    """the line the reference's run_binary writes for the recorded argument vector of `case`, our executable resolved"""
    ex = ARGV[case]["exec"]
    return "Calling: " + shlex.join([os.path.join(BIN, ex[0])] + ex[1:]) + "\n"


def test_reference_cli_execs_the_drop_in_hetmers(tmp_path):
    g = load_golden("k31_i1")
    case = "hetmers_pairs_t3_verbose"
    assert ARGV[case]["cli"] == ["hetmers", "-L", str(g["L"]), "-t", "3", "-o", "pairs", "--verbose", "t.ktab"]
    ktab.write_ktab(str(tmp_path / "t"), g["k"], g["packed"], g["counts"], ibyte=1, nparts=2)
    r = _cli(case, tmp_path)
    assert f"Calling: {BIN}/hetmers -opairs -e{g['L']} -T3 -v t.ktab\n" == _calling(case)
    assert _calling(case) in r.stderr, r.stderr
    assert "  The input table is trimmed and symmetric\n" in r.stderr          # our executable ran, and read the table
    from smudgeplot_amd import engine
    if engine.device_count() == 0:
        assert r.returncode != 0
        assert "hetmers: no HIP device available (this engine has no CPU fallback)" in r.stderr
        assert "CalledProcessError" in r.stderr                                 # run_binary's check=True, cli.py:72
        assert not (tmp_path / "pairs.smu").exists()
    else:
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "pairs.smu").read_text() == g["smu"]


def test_reference_cli_execs_the_drop_in_extract_and_reports_its_errors(tmp_path):
    r = _cli("extract_missing_table", tmp_path)
    assert f"Calling: {BIN}/extract_kmer_pairs -ox -T4 missing.ktab smudges\n" == _calling("extract_missing_table")
    assert _calling("extract_missing_table") in r.stderr, r.stderr
    assert r.returncode != 0 and "CalledProcessError" in r.stderr
    r = _cli("hetmers_missing_table", tmp_path)
    assert _calling("hetmers_missing_table") in r.stderr, r.stderr
    assert "hetmers: Cannot open k-mer table missing_table" in r.stderr         # the reference's message, PloidyPlot.c:1351-1354
    assert r.returncode != 0


def test_recorded_argv_is_what_the_documented_grammar_says():
    assert ARGV["hetmers_default"]["exec"] == ["hetmers", "-oOUT", "-e5", "-T4", "TABLE.ktab"]
    assert ARGV["hetmers_threads_verbose"]["exec"] == ["hetmers", "-oOUT", "-e12", "-T16", "-v", "TABLE.ktab"]
    assert ARGV["hetmers_tmp"]["exec"] == ["hetmers", "-oOUT", "-e4", "-T4", "-PTMPDIR", "TABLE"]
    assert ARGV["extract_verbose"]["exec"] == ["extract_kmer_pairs", "-oOUT", "-T8", "-v", "TABLE.ktab", "SMA"]


def _subst(argv, table, out, sma=None, tmp=None):
    m = {"TABLE.ktab": table + ".ktab", "TABLE": table, "SMA": sma or "SMA", "TMPDIR": tmp or "."}
    res = []
    for a in argv[1:]:
        if a.startswith("-o"):
            res.append("-o" + out)
        elif a.startswith("-P"):
            res.append("-P" + m["TMPDIR"])
        else:
            res.append(m.get(a, a))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["hetmers_default", "hetmers_threads_verbose", "hetmers_tmp"])
@pytest.mark.parametrize("name", ["k31_i1", "k51_i1_p3"])
def test_reference_cli_argv_replayed_on_the_drop_in_hetmers(case, name, tmp_path):
    g = load_golden(name)
    ktab.write_ktab(str(tmp_path / "t"), g["k"], g["packed"], g["counts"], ibyte=g["ibyte"], nparts=g["nparts"])
    argv = _subst(ARGV[case]["exec"], "t", "pairs", tmp=str(tmp_path))
    argv = [f"-e{g['L']}" if a.startswith("-e") else a for a in argv]         # (the golden tables are trimmed at their own L)
    r = subprocess.run([os.path.join(BIN, "hetmers"), *argv], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "pairs.smu").read_text() == g["smu"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["extract_default", "extract_verbose"])
def test_reference_cli_argv_replayed_on_the_drop_in_extract(case, tmp_path):
    from test_extract import load_extract, write_sma
    g, labels, lines, rows = load_extract("k31_i1")
    ktab.write_ktab(str(tmp_path / "t"), g["k"], g["packed"], g["counts"], ibyte=g["ibyte"], nparts=g["nparts"])
    write_sma(tmp_path / "s.sma", rows)
    argv = _subst(ARGV[case]["exec"], "t", "x", sma="s")
    r = subprocess.run([os.path.join(BIN, "extract_kmer_pairs"), *argv], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for lab, want in lines.items():
        got = sorted(open(tmp_path / f"x.{lab}.txt").read().splitlines(keepends=True))
        assert got == sorted(want), lab
