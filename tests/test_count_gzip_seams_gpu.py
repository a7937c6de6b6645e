"""Plain gzip on the GPU where the fixed sizes of csrc/smg_gzip.hpp and csrc/smg_count_inflater.hpp are reached: the kernels
byte by byte through count.gzip_inflate over gc.seam_streams() -- a full launch of 256 tasks and a piece that ends in every
kind of byte, decodes that run out of their 8 and their 64 ring slots, more than 4096 intervals and more than 64 MiB of text
in one file, more than 512 windows -- against gzip.decompress, then the host twin, then the report of the one against the
report of the other (tests/test_count_gzip_seams_host.py shows on the twin that each file reaches what it is made for); the
refusal of a distance in front of its member, which on the device is a flag the resolver sets; and three files on one reader
thread, whose windows lie in slabs beyond the first."""
import gzip

import pytest

import gzip_craft as gc
from smudgeplot_amd import count
from test_count_gzip_gpu import COUNTS, same

pytestmark = pytest.mark.gpu

CASES = [(name, span) for name, spans in gc.SEAM_SPANS.items() for span in spans]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, text); "<name>, plain": the text as a file"""
    d = tmp_path_factory.mktemp("gzip_seams")
    out = {}
    for i, (name, (data, want)) in enumerate(gc.seam_streams().items()):
        p = d / f"s{i}.fq.gz"
        p.write_bytes(data)
        out[name] = (str(p), want)
    p = d / "again.fq.gz"                                          # (an index is kept under the path of its file)
    p.write_bytes(gc.seam_streams()["many_members"][0])
    out["many_members, again"] = (str(p), out["many_members"][1])
    for name in ("many_members", "two_pieces"):
        p = d / f"{name}.fq"
        p.write_bytes(out[name][1])
        out[f"{name}, plain"] = (str(p), out[name][1])
    return out


@pytest.mark.parametrize("name,span", CASES, ids=[f"{name}-{span}" for name, span in CASES])
def test_the_kernels_give_the_text_of_gzip_and_the_report_of_the_twin_at_the_seams(name, span, files):
    path, want = files[name]
    got = count.gzip_inflate(path, span)[0]
    assert len(got) == len(want) and got == want
    dev = count.gzip_report(path)
    host_text = count.gzip_text_host(path, span)
    assert len(host_text) == len(want) and host_text == want
    host = count.gzip_report(path)
    print(name, span, dev)
    assert {c: dev[c] for c in COUNTS} == {c: host[c] for c in COUNTS}


@pytest.fixture(scope="module")
def reads():
    return gc.fastq_text(70_000, 1000)


@pytest.mark.parametrize("name", ["a far match in the first block of the file", "a far match behind four blocks",
                                  "a far match in the first block of a second member", "a far match behind four blocks of a second member"])
def test_a_distance_in_front_of_the_member_sets_the_flag_of_the_resolver(name, reads, tmp_path):
    data, off, why = gc.damaged_seams(reads)[name]
    with pytest.raises(Exception):
        gzip.decompress(data)
    bad, plain, good = tmp_path / "bad.fq.gz", tmp_path / "plain.fq", tmp_path / "good.fq.gz"
    bad.write_bytes(data)
    plain.write_bytes(reads)
    good.write_bytes(gc.gz(reads, 6, mem=1))
    for call in (lambda: count.gzip_inflate(str(bad), 1 << 10), lambda: count.gzip_inflate(str(bad), 64 << 10),
                 lambda: count.count_files([str(plain), str(bad)], 21, t=1, threads=2, gzip=True)):
        with pytest.raises(count.CountError) as e:
            call()
        assert e.value.code == -4 and f"{bad}: gzip member at offset {off}: {why}" in str(e.value), str(e.value)
        assert count.gzip_inflate(str(good), 1 << 10)[0] == reads   # the flag was cleared and nothing is left of the refusal


def test_three_files_on_one_reader_thread_fill_slabs_of_windows(files, monkeypatch):
    # One reader thread: one engine indexes the three files and keeps the windows of all of them, 512 to a slab.  Every
    # accepted decode takes one window at least, and many_members alone has more than 4096 + 300 of them (asserted on the twin
    # in tests/test_count_gzip_seams_host.py): more than 8 slabs.  So the windows of two_pieces begin in slab 8 or later, those
    # of the second many_members beyond them, and none of the second and third file has a number the first file of an engine has.
    monkeypatch.setenv("SMG_COUNT_GZIP_SPAN", "1024")
    names = ["many_members", "two_pieces", "many_members, again"]
    plain = count.count_files([files[f"{n.split(',')[0]}, plain"][0] for n in names], 21, t=1, threads=1)
    assert plain[0].counts.size > 100_000
    got = count.count_files([files[n][0] for n in names], 21, t=1, threads=1, gzip=True)
    same(got, plain)
    for n in names:
        r = count.gzip_report(files[n][0])
        print(n, r)
        assert r["text_bytes"] == len(files[n][1])
        assert n == "two_pieces" or r["linked"] + r["repaired"] > 8 * 512
