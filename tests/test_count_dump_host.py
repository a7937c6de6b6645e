"""K-mer dumps in front of the k-mer counter, without a GPU: the host twin of the line kernel (count.dump_parse: the cutter and
the line decoder that kd_lines compiles, run on the host) against the Python oracle of tests/dump_craft.py, each of the four
reasons a line is refused for with its offset, and the argument checks and refusals that need no device.
tests/test_count_dump_gpu.py holds the kernel against this twin.  (`make dump_check` runs the twin under the sanitizers at every
piece size and over mutated dumps; it takes a compiler and is run by hand, profiles/count_dump.md keeps its output.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dump_craft as dc
from conftest import ROOT
from smudgeplot_amd import count

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
COUNTS = [1, 32767, 32768, 4294967295, 4294967296, int("9" * 20), "007"]
DUMPS_ONLY = "a call with the dump option reads dumps only"


def test_the_binding_has_the_calls_the_field_and_the_line_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "smg_count.h")).read()
    assert {"smg_count_dump_parse", "smg_count_dump_records"} <= set(count.EXPORTS)
    assert re.search(r"int32_t gzip;[^}]*int32_t dump;[^}]*}\s*smg_count_opts;", hdr), "dump is the trailing field of the options"
    assert [n for n, _ in count.DumpOpts._fields_] == ["dump"] and issubclass(count.DumpOpts, count.Opts)
    assert count.DumpOpts.dump.offset == C.sizeof(count.Opts) == 24 and C.sizeof(count.DumpOpts) == 28
    o = count.DumpOpts(31, 4, 0, 2, 0, 1, 1)
    assert (o.kmer, o.minval, o.device, o.host_threads, o.verbose, o.gzip, o.dump) == (31, 4, 0, 2, 0, 1, 1)
    assert re.search(r"#define SMG_COUNT_DUMP_LINE\s+151\b", hdr) and count.DUMP_LINE == 151 == 128 + 1 + 20 + 2


@pytest.mark.parametrize("k", [13, 31, 32, 33, 64, 65, 96, 97, 128])
def test_dump_parse_gives_the_records_of_the_oracle(k, tmp_path):
    kmers = dc.random_kmers(k, 4 * len(COUNTS) + 3, seed=k, distinct_canonical=False)
    recs = []
    for i, s in enumerate(kmers):
        c = COUNTS[i % len(COUNTS)]
        sep = " " if i % 2 else "\t"
        end = "\r\n" if i % 3 == 0 else "\n"
        recs.append((s.lower() if i % 5 == 0 else s, c, sep, end))
    recs.append(("T" * k, 5, "\t", "\n"))                          # (canonical: a..a, the all-ones word where 2k is 64 j)
    recs.append((dc.revcomp(kmers[0]), 2, " ", "\n"))
    for last_end in (None, "", "\r"):
        p = tmp_path / f"d{k}_{len(last_end or 'n')}{'x' if last_end is None else ''}.txt"
        p.write_bytes(dc.text(recs, last_end=last_end))
        keys, cnts = count.dump_parse(p, k)
        want_k, want_c = dc.parse_oracle(recs)
        assert keys.shape == (len(recs), (k + 31) // 32) and cnts.dtype == np.uint32
        assert [tuple(int(x) for x in r) for r in keys] == want_k
        assert [int(c) for c in cnts] == want_c
    assert 4294967295 in want_c and want_c.count(4294967295) >= 3 and 7 in want_c


def test_an_empty_dump_has_no_records(tmp_path):
    p = tmp_path / "empty.txt"
    p.write_bytes(b"")
    keys, cnts = count.dump_parse(p, 31)
    assert keys.shape == (0, 1) and len(cnts) == 0


def bad_lines(k):
    """name -> (line, reason)"""
    s = "ACGT" * 33
    return {"one_base_short": (s[: k - 1] + "\t5\n", "bases"), "one_base_long": (s[: k + 1] + "\t5\n", "bases"),
            "an_n": (s[: k - 1] + "N\t5\n", "bases"), "comma": (s[:k] + ",5\n", "bases"), "blank": ("\n", "bases"),
            "no_count": (s[:k] + "\t\n", "nocount"), "two_separators": (s[:k] + "\t\t5\n", "nocount"), "minus": (s[:k] + " -5\n", "nocount"),
            "zero": (s[:k] + "\t0\n", "zero"), "zeros": (s[:k] + " 000\r\n", "zero"),
            "21_digits": (s[:k] + "\t" + "1" * 21 + "\n", "noend"), "a_point": (s[:k] + "\t5.0\n", "noend"),
            "trailing_blank": (s[:k] + "\t5 \n", "noend"), "cr_only": (s[:k] + "\t5\rA\n", "noend")}


@pytest.mark.parametrize("k", [21, 128])
def test_every_reason_with_its_offset_on_the_first_a_middle_and_the_last_line(k, tmp_path):
    good = [dc.line(s, 3 + i) for i, s in enumerate(dc.random_kmers(k, 40, seed=2))]
    for name, (bad, reason) in bad_lines(k).items():
        for at in (0, 17, 40):
            if name == "blank" and at == 0:                       # (a text that begins with no base is no dump at all: below)
                continue
            lines = good[:at] + [bad.encode()] + good[at:]
            if at == 17:
                lines.insert(30, b"ACGT\n")                       # (a later bad line: the first one is reported)
            p = tmp_path / f"{name}_{at}.txt"
            p.write_bytes(b"".join(lines))
            with pytest.raises(count.CountError) as e:
                count.dump_parse(p, k)
            off = sum(len(x) for x in good[:at])
            assert e.value.code == -4, (name, at, str(e.value))
            assert str(e.value).endswith(f"{p}: dump line at offset {off}: {dc.REASONS[reason].format(k=k)}"), (name, at, str(e.value))
    # the last line without its line end, and a line far longer than any legal one
    p = tmp_path / "cut.txt"
    p.write_bytes(b"".join(good) + ("ACGT" * 32)[:k].encode() + b"\t")
    with pytest.raises(count.CountError) as e:
        count.dump_parse(p, k)
    assert str(e.value).endswith(f"offset {sum(map(len, good))}: has no count")
    p.write_bytes(b"".join(good[:5]) + ("ACGT" * 32)[:k].encode() + b"\t" + b"7" * 100000 + b"\n" + b"".join(good))
    with pytest.raises(count.CountError) as e:
        count.dump_parse(p, k)
    assert str(e.value).endswith(f"offset {sum(map(len, good[:5]))}: count is not followed by a line end")


def test_what_is_no_dump_is_refused_by_name(tmp_path):
    for name, data in (("r.fa", b">a\nACGTACGTACGTACGTACGT\n"), ("r.fq", b"@a\nACGT\n+\nIIII\n"), ("r.txt", b"# k-mer\tcount\n"),
                       ("n.txt", b"NACGT 4\n")):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(count.CountError) as e:
            count.dump_parse(p, 21)
        assert e.value.code == -2 and str(p) in str(e.value) and DUMPS_ONLY in str(e.value)
        with pytest.raises(count.CountError) as e:                  # refused before the device is looked for
            count.count_files(p, 21, dump=True)
        assert e.value.code == -2 and str(p) in str(e.value) and DUMPS_ONLY in str(e.value)
    with pytest.raises(count.CountError) as e:
        count.dump_parse(tmp_path / "absent.txt", 21)
    assert "cannot open" in str(e.value)
    for k in (12, 129):
        with pytest.raises(count.CountError) as e:
            count.dump_parse(tmp_path / "r.txt", k)
        assert e.value.code == -2 and "out of range" in str(e.value)


def test_a_dump_is_counted_in_one_pass_only(tmp_path):
    p = tmp_path / "d.txt"
    p.write_bytes(dc.line("ACGTACGTACGTACGTACGTA", 4))
    for parts in (2, 4096):
        with pytest.raises(count.CountError) as e:
            count.count_files(p, 21, dump=True, partitions=parts)
        assert e.value.code == -2 and "partitions must be 0 or 1" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        count.reads_to_plot(b"ACGT", 21, 1, 1, dump=True)


def run(args, cwd):
    return subprocess.run([COUNT_BIN, *args], cwd=cwd, capture_output=True, text=True)


def test_smg_count_has_the_option_and_refuses_reads_under_it(tmp_path):
    (tmp_path / "r.fa").write_bytes(b">a\nACGTACGTACGTACGTACGTACGT\n")
    r = run([], tmp_path)
    assert r.returncode == 1 and "Usage: smg_count [-v] [-g] [-d]" in r.stderr and "-d: the inputs are k-mer dumps" in r.stderr
    r = run(["-k21", "-d", "-H", "r.fa"], tmp_path)
    assert r.returncode == 1 and "illegal option" not in r.stderr, r.stderr
    assert "r.fa is not a k-mer dump" in r.stderr and DUMPS_ONLY in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["r.fa"]
    r = run(["-k21", "-z", "-d", "r.fa"], tmp_path)
    assert r.returncode == 1 and "-z is an illegal option" in r.stderr
    (tmp_path / "d.txt").write_bytes(dc.line("ACGTACGTACGTACGTACGTA", 4))
    r = run(["-k21", "-d", "-p2", "d.txt"], tmp_path)
    assert r.returncode == 1 and "partitions must be 0 or 1" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["d.txt", "r.fa"]
