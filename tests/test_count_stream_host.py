"""Streams in front of the k-mer counter, no GPU: a FIFO (os.mkfifo, a writer thread that writes in pieces) through the host
calls against the same bytes in a regular file, the refusals, the plan of a run without a bound (count.stream_plan) over a
grid, and the argument errors of the `smg_count` executable that come before any device is needed.  (The reader under the
sanitizers, streams included, is `make reader_check`, run by hand; profiles/count_stream.md keeps its output.)"""
import gzip
import itertools
import os
import subprocess
import sys

import pytest

import bgzf_craft as bz
import dump_craft as dc
from fifo_craft import Writer, refused, through_fifo
from smudgeplot_amd import count

PIECES = [1, 7, 65537]
TILE = 4096


def fastq(n, crlf=False, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    recs = []
    for i in range(n):
        s = (b"ACGTTGCAnNacgt" * 12)[i % 11:i % 11 + 40 + i % 97]
        recs.append(b"@r%d" % i + nl + s + nl + b"+" + nl + b"I" * len(s) + nl)
    text = b"".join(recs)
    return text if final_newline else text[:-len(nl)]


def fasta(n, crlf=False, final_newline=True):
    nl = b"\r\n" if crlf else b"\n"
    text = b"".join(b">s%d some text" % i + nl + b"".join((b"ACGGTCA" * 40)[j:j + 60] + nl for j in range(0, 100 + i % 150, 60)) for i in range(n))
    return text if final_newline else text[:-len(nl)]


INPUTS = {
    "fastq": fastq(1500),
    "fasta_multiline": fasta(700),
    "fastq_crlf": fastq(900, crlf=True),
    "fasta_crlf_no_final_newline": fasta(300, crlf=True, final_newline=False),
    "fastq_no_final_newline": fastq(50, final_newline=False),
    "empty": b"",
    "shorter_than_a_bgzf_header": b">r\nACGT\nAC",
    "one_byte": b">",
}
assert all(len(INPUTS[n]) > 2 * 65537 for n in ("fastq", "fasta_multiline", "fastq_crlf"))      # (several of the largest pieces)


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_parse_of_a_fifo_equals_parse_of_the_file(name, piece, tmp_path):
    data = INPUTS[name]
    if piece == 1:
        data = data[:20000]                                      # (byte by byte: a part is enough, and it ends inside a record)
    p = tmp_path / "in.txt"
    p.write_bytes(data)
    want = count.parse(p)
    assert through_fifo(tmp_path, data, piece, count.parse) == want
    assert name in ("empty", "one_byte") or len(want) > 0


def test_parse_of_standard_input_and_of_dev_stdin(tmp_path):
    """"-" is standard input; /dev/stdin is a stream by fstat (a pipe here)"""
    data = INPUTS["fastq"]
    p = tmp_path / "in.fq"
    p.write_bytes(data)
    want = count.parse(p)
    prog = ("import sys; from smudgeplot_amd import count; sys.stdout.buffer.write(count.parse(sys.argv[1]))")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(count.__file__)))] +
                                                      os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    for arg in ("-", "/dev/stdin"):
        r = subprocess.run([sys.executable, "-c", prog, arg], input=data, capture_output=True, env=env, timeout=60)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, arg


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("k", [31, 65])
def test_dump_parse_of_a_fifo_equals_the_records_of_the_file(k, piece, tmp_path):
    kmers = dc.random_kmers(k, 2500, seed=k, distinct_canonical=False)
    data = dc.text([(s, 1 + 37 * i) for i, s in enumerate(kmers)], last_end="")
    assert len(data) > 65537
    p = tmp_path / "d.txt"
    p.write_bytes(data)
    hk, hc = count.dump_parse(p, k)
    fk, fc = through_fifo(tmp_path, data, piece, lambda f: count.dump_parse(f, k))
    assert len(hc) == 2500 and fk.tolist() == hk.tolist() and fc.tolist() == hc.tolist()


def test_gzip_and_bgzf_on_a_fifo_get_the_refusals_of_the_files(tmp_path):
    text = INPUTS["fastq"][:5000]
    for data, words, call in ((gzip.compress(text), "is gzip compressed: compressed input is not supported, decompress it first", count.parse),
                              (bz.bgzf(text), "is BGZF compressed: this call has no device to inflate it on, use smg_count_bgzf_inflate or one of "
                                              "the counting calls", count.parse),
                              (bz.bgzf(b"ACGTACGTACGTACGTACGTA\t3\n"), "is BGZF compressed: this call has no device to inflate it on, use one of the "
                                                                        "counting calls or smg_count_dump_records", lambda f: count.dump_parse(f, 21))):
        p = tmp_path / "in.gz"
        p.write_bytes(data)
        with pytest.raises(count.CountError) as of_file:
            call(str(p))
        e = refused(tmp_path, data, call)
        assert e.code == of_file.value.code == -2
        assert str(e) == f"smg_count error -2: {tmp_path / 'bad.fifo'} {words}"
        assert str(of_file.value) == f"smg_count error -2: {p} {words}"


def test_the_file_tools_refuse_a_stream_without_opening_it(tmp_path):
    """they read a file twice or seek in it; the refusal is by stat, which opens nothing: the writer that waits for a reader
    of the FIFO (it is there so that a call that did open it would not wait for ever) still waits when all have answered"""
    fifo = tmp_path / "nobody_reads.fifo"
    os.mkfifo(fifo)
    calls = {"bgzf_scan": count.bgzf_scan, "bgzf_inflate": count.bgzf_inflate, "bam_strip": count.bam_strip,
             "gzip_inflate": count.gzip_inflate, "gzip_text_host": count.gzip_text_host}
    w = Writer(fifo, b"", 1)
    try:
        for path in ("-", str(fifo)):
            for name, call in calls.items():
                with pytest.raises(count.CountError) as e:
                    call(path)
                assert e.value.code == -2 and str(e.value) == f"smg_count error -2: {path} is a stream: this call reads a file", name
        assert w.is_alive(), "a file tool opened the FIFO"
    finally:
        w.finish(0)


# ---- the plan of a run without a bound ------------------------------------------------------------------------------------

def batch_price(k):
    w = (k + 31) // 32
    return 1 + 16 * w + 12 + (24 if w > 1 else 0)


def tiles(n):
    return -(-n // TILE) * TILE


GB = 1 << 30
GRID = list(itertools.product([13, 31, 32, 33, 51, 128], [3 * GB, 64 * GB, 288 * GB], [0, 1000, 5 * GB], [0, 1, 2, 3, 4096], [0, 1000],
                              [0, 8192], [0, 1, 4096, 4097, 200000]))


def test_stream_plan_over_a_grid():
    for k, free, known, parts, max_entries, batch, store in GRID:
        what = (k, free, known, parts, max_entries, batch, store)
        first = 0
        if parts != 1:                                           # the store: the hook in whole tiles, else 2^30 or what the files need
            first = tiles(store) if store else tiles(max(1 << 30, known + known // 32 + (1 << 16)))
        left = free - first // 8 * 3
        cap = min(left // 3 // batch_price(k), 1 << 30) if not batch else batch + k
        cap = max(cap, k + 1)
        fits = (parts == 1 or first // 8 * 3 + (64 << 20) <= free) and cap * batch_price(k) <= left
        if not fits:
            with pytest.raises(count.CountError) as e:
                count.stream_plan(k, free, known, parts, max_entries, batch, store)
            assert e.value.code == -3 and "GB" in str(e.value), what
            continue
        got = count.stream_plan(k, free, known, parts, max_entries, batch, store)
        assert got == {"cap": cap, "parted": parts != 1, "store_cap": first}, what
        assert got["store_cap"] % TILE == 0
        # the batch never clamps to the input: that of memory_plan over the same bytes does where they are few
        if known == 1000 and not batch and parts == 1 and not max_entries:
            assert count.memory_plan(k, free, known, 1)["cap"] == known + k + 1 < got["cap"], what


def test_stream_plan_rounds_the_store_as_memory_plan_does():
    for bound in (0, 1, 4095, 4096, 70000, 10 ** 9):
        mp = count.memory_plan(31, 64 * GB, bound, partitions=2)
        assert mp["parted"] and mp["store_cap"] == tiles(bound + bound // 32 + (1 << 16))
        # a store asked for by the hook at the size memory_plan gave comes back as it is; one position more is one tile more
        assert count.stream_plan(31, 64 * GB, 0, 0, store_bases=mp["store_cap"])["store_cap"] == mp["store_cap"]
        assert count.stream_plan(31, 64 * GB, 0, 0, store_bases=mp["store_cap"] + 1)["store_cap"] == mp["store_cap"] + TILE
    # without the hook the regular files of the call are in the first size, as memory_plan sizes them
    big = 40 * GB
    assert count.stream_plan(31, 288 * GB, big, 0)["store_cap"] == count.memory_plan(31, 288 * GB, big, partitions=2)["store_cap"]


def test_with_no_stream_in_the_call_memory_plan_decides():
    """both plans over one bound: memory_plan takes one pass where the bound guarantees that it fits and clamps the batch to the
    input; stream_plan, which trusts no bound, packs.  The counting calls take memory_plan's unless a stream is among the
    inputs, and say so where they are documented."""
    mp = count.memory_plan(31, 64 * GB, 10 ** 6)
    sp = count.stream_plan(31, 64 * GB, 10 ** 6)
    assert mp == {"cap": 10 ** 6 + 32, "parted": False, "store_cap": 0}
    assert sp["parted"] and sp["store_cap"] == 1 << 30 and sp["cap"] > mp["cap"]
    assert "With no stream in the call it is memory_plan that decides" in " ".join(count.stream_plan.__doc__.split())
    hdr = " ".join(open(os.path.join(os.path.dirname(count.__file__), "..", "include", "smg_count.h")).read().split())
    assert "With no stream in the call smg_count_memory_plan decides" in hdr


@pytest.mark.parametrize("bad", [dict(k=12), dict(k=129), dict(known_bound=-1), dict(partitions=-1), dict(partitions=4097), dict(max_entries=-1),
                                 dict(store_bases=-1)])
def test_stream_plan_refuses_bad_arguments(bad):
    args = dict(k=31, free_bytes=64 * GB, known_bound=0, partitions=0, max_entries=0, batch_bases=0, store_bases=0)
    args.update(bad)
    with pytest.raises(count.CountError) as e:
        count.stream_plan(**args)
    assert e.value.code == -2


# ---- the executable, up to where it needs a device --------------------------------------------------------------------------

def run(args, cwd, **kw):
    """(the time limit is for an executable that opens a FIFO nobody writes to: it would wait for ever)"""
    return subprocess.run([count.BIN_PATH, *args], cwd=cwd, capture_output=True, text=True, timeout=20, **kw)


def test_smg_count_wants_a_root_name_where_the_first_input_is_a_stream(tmp_path):
    os.mkfifo(tmp_path / "reads.fifo")
    (tmp_path / "r.fa").write_bytes(b">a\nACGTACGTACGTACGTACGTACGT\n")
    for first in ("-", "/dev/stdin", "reads.fifo"):
        r = run(["-k21", first, "r.fa"], tmp_path, stdin=subprocess.DEVNULL)
        assert r.returncode == 1 and r.stderr == f"smg_count: -o is needed where the first input is a stream ({first})\n"
    assert sorted(os.listdir(tmp_path)) == ["r.fa", "reads.fifo"]


def test_smg_count_reads_standard_input_once(tmp_path):
    r = run(["-k21", "-oX", "-", "-"], tmp_path, stdin=subprocess.DEVNULL)
    assert r.returncode == 1 and r.stderr == "smg_count: - (standard input) is named twice: it can be read once\n"
    assert os.listdir(tmp_path) == []
    with pytest.raises(count.CountError) as e:
        count.count_files(["-", str(tmp_path / "r.fa"), "-"], 21)
    assert e.value.code == -2 and "- (standard input) is named twice" in str(e.value)


def test_smg_count_does_not_open_a_fifo_before_the_run(tmp_path):
    """The check of the arguments is stat and access for what is no regular file: opening and closing a FIFO would end its
    writer.  The writer here writes all it has in one piece once somebody reads, and sees no closed pipe; the run then goes
    as far as the machine allows -- to the table, or to the refusal for want of a device -- and leaves nothing behind it
    where it failed.  (With a check that opened the FIFO the run would wait for a second writer that never comes.)"""
    os.mkfifo(tmp_path / "reads.fifo")
    data = b"".join(b">r%d\nACGTTGCATTGACCAGTACGATCAGGAT\n" % i for i in range(20))
    w = Writer(tmp_path / "reads.fifo", data, len(data))
    try:
        r = run(["-k21", "-t1", "-oX", "reads.fifo"], tmp_path)
    finally:
        w.finish()
    assert w.error is None and w.wrote == len(data)
    if r.returncode == 0:
        assert sorted(os.listdir(tmp_path)) == [".X.ktab.1", "X.ktab", "reads.fifo"]
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, r.stderr
        assert os.listdir(tmp_path) == ["reads.fifo"]
    absent = run(["-k21", "-oX", "reads.fifo", "no_such_file"], tmp_path)
    assert absent.returncode == 1 and "Cannot open no_such_file for reading" in absent.stderr
