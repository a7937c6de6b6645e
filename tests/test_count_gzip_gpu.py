"""Plain gzip in front of the k-mer counter on the GPU: the four kernels byte by byte through count.gzip_inflate at the smallest
spans (the oracle is gzip.decompress; tests/test_count_gzip_host.py holds the same streams against the host twin, and
`make gzip_check` has held the twin against zlib on the CPU), their report against the twin's, counting with gzip=True against
the plain run, the executable with -g, and a damaged member.  Every stream here is some 300 KB at ordinary ratios, so hardly
one of the fixed sizes of the code is reached: tests/test_count_gzip_seams_gpu.py has the files that fill a piece, the ring
slots of a decode, a slab of windows, and the intervals and the text of one call, and the refusal of the resolver."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_craft as bz
import gzip_craft as gc
from smudgeplot_amd import count

pytestmark = pytest.mark.gpu

NAMES = ["level1", "level6", "level9", "fixed", "stored", "huffman_only", "rle", "memlevel1", "sync_flush", "two_members", "fifty_members",
         "header_fields", "trailing_zeros", "far_match", "gzip_in_gzip"]
COUNTS = ("members", "text_bytes", "spans", "linked", "repaired")


@pytest.fixture(scope="module")
def text():
    return gc.fastq_text()


@pytest.fixture(scope="module")
def files(text, tmp_path_factory):
    """name -> (path, text); and the same reads as a plain and as a BGZF file"""
    d = tmp_path_factory.mktemp("gzip")
    out = {}
    for name, (data, want) in gc.streams(text).items():
        p = d / f"{name}.fq.gz"
        p.write_bytes(data)
        out[name] = (str(p), want)
    (d / "plain.fq").write_bytes(text)
    (d / "bgzf.fq.gz").write_bytes(bz.bgzf(text))
    out["plain"] = (str(d / "plain.fq"), text)
    out["bgzf"] = (str(d / "bgzf.fq.gz"), text)
    return out


@pytest.mark.parametrize("span", [1 << 10, 4 << 10])
@pytest.mark.parametrize("name", NAMES)
def test_the_kernels_give_the_text_of_gzip_and_the_report_of_the_twin(name, span, files):
    path, want = files[name]
    assert gzip.decompress(open(path, "rb").read()) == want
    got, ms = count.gzip_inflate(path, span)
    assert got == want
    dev = count.gzip_report(path)
    assert len(ms) == 3 and ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and (dev["ms_marker"], dev["ms_resolve"], dev["ms_exact"]) == ms
    assert count.gzip_text_host(path, span) == want
    host = count.gzip_report(path)
    print(name, span, dev)
    assert {c: dev[c] for c in COUNTS} == {c: host[c] for c in COUNTS}


def test_a_span_larger_than_the_file_and_the_default(files):
    path, want = files["level6"]
    for span in (1 << 20, 0):
        assert count.gzip_inflate(path, span)[0] == want
        assert count.gzip_report(path)["spans"] == 1


def same(got, want):
    assert np.array_equal(got[0].packed, want[0].packed) and np.array_equal(got[0].counts, want[0].counts) and np.array_equal(got[1], want[1])
    assert got[2]["bases"] == want[2]["bases"]


@pytest.mark.parametrize("partitions", [1, 3])
@pytest.mark.parametrize("k", [21, 40])
def test_counting_from_gzip_equals_the_plain_run(k, partitions, files, monkeypatch):
    monkeypatch.setenv("SMG_COUNT_GZIP_SPAN", "1024")
    plain = count.count_files(files["plain"][0], k, t=1, threads=1, partitions=partitions)
    assert plain[0].counts.size > 10_000
    for name in ("level6", "fifty_members"):
        got = count.count_files([files[name][0]], k, t=1, threads=1, partitions=partitions, gzip=True)
        same(got, plain)
        assert got[2]["used"] == partitions
        assert count.gzip_report(files[name][0])["text_bytes"] == len(files[name][1])
    same(count.count_files(files["plain"][0], k, t=1, threads=1, partitions=partitions, gzip=True), plain)     # (the option changes nothing for it)


def test_plain_bgzf_and_gzip_files_on_two_reader_threads(files, monkeypatch):
    monkeypatch.setenv("SMG_COUNT_GZIP_SPAN", "4096")
    three = count.count_files([files["plain"][0]] * 3, 21, t=2, threads=2)
    for order in (["plain", "bgzf", "memlevel1"], ["rle", "plain", "bgzf"]):
        same(count.count_files([files[n][0] for n in order], 21, t=2, threads=2, gzip=True), three)
    with pytest.raises(count.CountError) as e:                   # the option off: the gzip file of the list is refused as always
        count.count_files([files[n][0] for n in ("plain", "bgzf", "memlevel1")], 21, t=2, threads=2)
    assert e.value.code == -2 and "is gzip compressed: compressed input is not supported" in str(e.value)


def test_the_executable_with_g_writes_what_the_plain_run_writes(files, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    reads = gc.het_fastq()                                      # (reads with het-mer pairs, so that the .smu holds something)
    (a / "reads.fq").write_bytes(reads)
    (b / "reads.fq.gz").write_bytes(gc.gz(reads[:70_000], 6) + gc.gz(reads[70_000:], 1))
    env = dict(os.environ, SMG_COUNT_GZIP_SPAN="1024")
    for d, args in ((a, ["reads.fq"]), (b, ["-g", "reads.fq.gz"])):
        r = subprocess.run([count.BIN_PATH, "-k21", "-t1", "-H", "-v", *args], cwd=d, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        if "-g" in args:
            assert f"reads.fq.gz: gzip, 2 members, {len(reads)} text bytes, " in r.stderr and "repaired, inflated on the device" in r.stderr
    for name in ("reads.ktab", ".reads.ktab.1", "reads.hist.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    assert (a / "reads.hist.txt").stat().st_size > 0
    for d, args in ((a, ["reads.fq"]), (b, ["-g", "reads.fq.gz"])):
        r = subprocess.run([count.BIN_PATH, "-k21", "-t2", "-e2", "-n", *args], cwd=d, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
    assert (a / "reads.smu").read_bytes() == (b / "reads.smu").read_bytes() and (a / "reads.smu").stat().st_size > 0
    r = subprocess.run([count.BIN_PATH, "-k21", "-t1", "-orefused", "reads.fq.gz"], cwd=b, capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "is gzip compressed: compressed input is not supported" in r.stderr
    assert not [n for n in os.listdir(b) if "refused" in n]


@pytest.mark.parametrize("name", ["a flipped text byte in a stored block", "cut inside a block", "a wrong ISIZE in the second member"])
def test_a_damaged_member_under_g_is_refused_with_its_offset_and_nothing_is_written(name, text, files, tmp_path):
    data, off, why = gc.damaged(text)[name]
    d = tmp_path / "run"
    d.mkdir()
    path = d / "bad.fq.gz"
    path.write_bytes(data)
    where = "deflate block at offset " if off is None else f"gzip member at offset {off}: "
    for call in (lambda: count.gzip_inflate(str(path), 1 << 10), lambda: count.count_files([files["plain"][0], str(path)], 21, t=1, threads=2, gzip=True)):
        with pytest.raises(count.CountError) as e:
            call()
        assert e.value.code == -4 and f"{path}: {where}" in str(e.value) and why in str(e.value), str(e.value)
    r = subprocess.run([count.BIN_PATH, "-g", "-k21", "-t1", "-H", "bad.fq.gz"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 1 and where in r.stderr and why in r.stderr, r.stderr
    assert sorted(os.listdir(d)) == ["bad.fq.gz"]
    good = count.count_files([files["level1"][0]], 21, t=1, threads=1, gzip=True)      # a valid run afterwards, in the same process
    assert good[2]["bases"] > 50_000
