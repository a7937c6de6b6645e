"""Reads to .smu in one process, the host side (no GPU): the new options of `smg_count` refuse what they cannot do before
anything is written, and the two libraries export what their headers and bindings say -- the counter's library nothing of the
engine's."""
import os
import re
import subprocess

from conftest import LIB, ROOT
from smudgeplot_amd import count, engine

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
COUNT_LIB = os.path.join(ROOT, "smudgeplot_amd", "libsmg_count.so")


def run(args, cwd):
    return subprocess.run([COUNT_BIN, *args], cwd=cwd, capture_output=True, text=True)


def reads(tmp_path):
    (tmp_path / "r.fa").write_bytes(b">a\nACGTACGTACGTACGTACGTACGTAGCTAGCTAGGATCGAT\n")


def test_no_table_alone_is_a_usage_error(tmp_path):
    reads(tmp_path)
    r = run(["-k21", "-n", "r.fa"], tmp_path)
    assert r.returncode == 1, r.stderr
    assert "-n leaves nothing to write" in r.stderr and "Usage: smg_count" in r.stderr and "-e<int>" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["r.fa"]


def test_e_below_t_is_refused(tmp_path):
    reads(tmp_path)
    for args in (["-k21", "-e3", "-t4", "r.fa"], ["-k21", "-e3", "r.fa"], ["-k21", "-t4", "-e3", "-n", "-H", "r.fa"]):
        r = run(args, tmp_path)
        assert r.returncode == 1, (args, r.stderr)
        assert "-e3 is below -t4" in r.stderr and "not counted into the table" in r.stderr, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["r.fa"], args


def test_e_wants_a_positive_integer(tmp_path):
    reads(tmp_path)
    for arg, msg in (("-ex", "argument is not an integer"), ("-e", "argument is not an integer"), ("-e0", "must be positive")):
        r = run(["-k21", arg, "r.fa"], tmp_path)
        assert r.returncode == 1 and msg in r.stderr, (arg, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["r.fa"], arg


def test_both_libraries_export_what_their_headers_declare():
    for header, lib, exports, pattern in (("smg_count.h", COUNT_LIB, count.EXPORTS, r"smg_count_[a-z0-9_]+"),
                                          ("smg_hetmers.h", LIB, engine.EXPORTS, r"smg_[a-z0-9_]+")):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        declared = set(re.findall(r"\b(" + pattern + r")\s*\(", hdr))
        assert declared == set(exports), header
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        defined = set(re.findall(r" T (smg_[a-z0-9_]+)$", out, flags=re.M))
        assert defined == declared, header
    assert {"smg_count_files_device", "smg_count_bases_device", "smg_count_device_free"} <= set(count.EXPORTS)
    assert {"smg_engine_close_canonical", "smg_engine_merge_tile", "smg_hetmers_run_device"} <= set(engine.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", COUNT_LIB], capture_output=True, text=True, check=True).stdout
    assert not re.search(r" T smg_(engine|hetmers)_", out)          # the counter's library holds nothing of the engine


def test_merge_tiles_need_no_device():
    """the tile of the merge kernel per key width, from the library: what test_close_canonical_gpu.py cuts its tables at"""
    tiles = [engine.merge_tile(w) for w in (1, 2, 3, 4)]
    assert all(t >= 256 and t % 256 == 0 for t in tiles), tiles
    # 8 W + 2 bytes of LDS per output: at least two workgroups in the 160 KiB of a CU
    assert all(2 * t * (8 * w + 2) <= 160 * 1024 for w, t in zip((1, 2, 3, 4), tiles))
    assert engine.merge_tile(0) == 0 and engine.merge_tile(5) == 0


def test_reads_to_plot_refuses_e_below_t_before_it_counts():
    import pytest
    with pytest.raises(ValueError, match="below t"):
        count.reads_to_plot(b"ACGT" * 20, 21, 4, 3)
