"""K-mer dumps in front of the k-mer counter on the GPU: the line kernel record by record against its host twin
(count.dump_records against count.dump_parse, which tests/test_count_dump_host.py holds against the Python oracle) where a
tile, its halo and a batch end; its refusals with the message and the offset of the twin; counting with dump=True against
the oracle of tests/dump_craft.py where sums saturate, runs outgrow a workgroup and 65535, and a k-mer meets itself across
merges; the round trip reads -> table -> dump -> table, to the .smu; and compressed dumps.  Every input is small: some
hundred thousand lines at the most."""
import os
import random
import subprocess

import numpy as np
import pytest

import bgzf_craft as bz
import dump_craft as dc
import gzip_craft as gc
from conftest import ROOT
from smudgeplot_amd import count

pytestmark = pytest.mark.gpu

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
TILE = 4096


def padded(k, kmers, target):
    """lines of the k-mers (count 7 with leading zeros) whose lengths add up to `target` exactly -> (bytes, k-mers used)"""
    lo, hi = k + 3, k + 22                                          # a line with 1 .. 20 digits
    m = -(-target // hi)
    assert m * lo <= target <= m * hi and m <= len(kmers), (k, target)
    sizes = [target // m + (1 if i < target % m else 0) for i in range(m)]
    return b"".join(dc.line(kmers[i], "7".rjust(n - k - 2, "0")) for i, n in enumerate(sizes)), m


def same_records(path, k, gzip_on=False):
    """dump_records equals dump_parse as sorted lists; -> the number of records"""
    hk, hc = count.dump_parse(path, k) if not gzip_on else (None, None)
    dk, dcn, ms = count.dump_records(path, k, gzip=gzip_on)
    if hk is None:
        return dk, dcn
    assert dk.shape == hk.shape and len(dcn) == len(hc)
    host = sorted(zip(map(tuple, hk.tolist()), hc.tolist()))
    dev = sorted(zip(map(tuple, dk.tolist()), dcn.tolist()))
    assert dev == host
    assert ms >= 0
    return len(hc)


@pytest.mark.parametrize("k", [31, 64, 96, 128])
def test_records_of_the_kernel_are_those_of_the_twin_where_a_tile_ends(k, tmp_path):
    kmers = dc.random_kmers(k, 400, seed=k, distinct_canonical=False)
    p = tmp_path / "d.txt"
    p.write_bytes(b"")
    assert same_records(p, k) == 0
    p.write_bytes(dc.line(kmers[0], 4294967296, " ", "\r\n"))
    assert same_records(p, k) == 1
    p.write_bytes(dc.line(kmers[0], 12, "\t", ""))                  # (no line end at the end of the text)
    assert same_records(p, k) == 1
    for size in (1000, TILE, TILE + 1, 3 * TILE - 1):
        text, n = padded(k, kmers, size)
        assert len(text) == size
        p.write_bytes(text)
        assert same_records(p, k) == n
    # a line start on the last byte of a tile, on the first of the next and on the one behind it; in the second tile too
    for start in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        head, n = padded(k, kmers, start)
        tail = b"".join(dc.line(s, 1 + i, " ") for i, s in enumerate(kmers[n: n + 40]))
        p.write_bytes(head + tail)
        assert same_records(p, k) == n + 40


def test_a_longest_line_that_starts_on_the_last_byte_of_a_tile(tmp_path):
    k = 128
    kmers = dc.random_kmers(k, 100, seed=9, distinct_canonical=False)
    longest = dc.line(kmers[99].lower(), "9" * 20, "\t", "\r\n")
    assert len(longest) == count.DUMP_LINE
    p = tmp_path / "d.txt"
    for start in (TILE - 1, 2 * TILE - 1):
        head, n = padded(k, kmers, start)
        for behind in (b"", dc.line(kmers[98], 3)):
            p.write_bytes(head + longest + behind)
            assert same_records(p, k) == n + 1 + (1 if behind else 0)
            dk, dcn, _ = count.dump_records(p, k)
            assert 4294967295 in dcn.tolist()
        # one byte more is one too many, for the twin and for the kernel alike
        p.write_bytes(head + longest[:-2] + b"9\r\n")
        msgs = []
        for call in (count.dump_parse, count.dump_records):
            with pytest.raises(count.CountError) as e:
                call(p, k)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1] and msgs[0].endswith(f"offset {start}: count is not followed by a line end")


def device_and_twin_refuse(path, k, **kw):
    with pytest.raises(count.CountError) as e:
        count.dump_parse(path, k)
    with pytest.raises(count.CountError) as d:
        count.dump_records(path, k)
    assert d.value.code == e.value.code == -4 and str(d.value) == str(e.value)
    with pytest.raises(count.CountError) as c:
        count.count_files(path, k, t=1, dump=True, **kw)
    assert str(c.value) == str(e.value)
    return str(e.value)


def test_bad_lines_are_refused_as_the_twin_refuses_them(tmp_path, monkeypatch):
    k = 31
    kmers = dc.random_kmers(k, 600, seed=4)
    good = [dc.line(s, 3 + i) for i, s in enumerate(kmers)]
    s = kmers[0]
    bad = {"bases": s[:-1] + "\t5\n", "nocount": s + "\t\t5\n", "zero": s + " 00\n", "noend": s + " " + "1" * 21 + "\n"}
    p = tmp_path / "d.txt"
    for reason, line in bad.items():
        for at in (0, 300, 600):
            p.write_bytes(b"".join(good[:at]) + line.encode() + b"".join(good[at:]))
            msg = device_and_twin_refuse(p, k)
            assert msg.endswith(f"offset {sum(map(len, good[:at]))}: {dc.REASONS[reason].format(k=k)}")
    # two bad lines in different tiles: the earlier one is reported
    lines = list(good)
    lines[150] = bad["zero"].encode()
    lines[500] = bad["bases"].encode()
    assert sum(map(len, lines[:150])) // TILE < sum(map(len, lines[:500])) // TILE
    p.write_bytes(b"".join(lines))
    assert device_and_twin_refuse(p, k).endswith(f"offset {sum(map(len, lines[:150]))}: count is 0")
    # a bad line in a later batch, and a last line that the end of the text cuts
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", "4096")
    assert device_and_twin_refuse(p, k).endswith(f"offset {sum(map(len, lines[:150]))}: count is 0")
    lines[150] = good[150]
    assert sum(map(len, lines[:500])) > 3 * 4096
    p.write_bytes(b"".join(lines))
    assert device_and_twin_refuse(p, k).endswith(f"offset {sum(map(len, lines[:500]))}: {dc.REASONS['bases'].format(k=k)}")
    p.write_bytes(b"".join(good) + s.encode() + b" ")
    assert device_and_twin_refuse(p, k).endswith(f"offset {sum(map(len, good))}: has no count")
    # a line longer than a whole batch
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", "100")
    p.write_bytes(b"".join(good[:7]) + s.encode() + b" " + b"5" * 5000 + b"\n" + b"".join(good))
    assert device_and_twin_refuse(p, k).endswith(f"offset {sum(map(len, good[:7]))}: count is not followed by a line end")


def counted(paths, k, t, records, **kw):
    """count_files(dump=True) against the oracle: table, hist, stats"""
    tab, hist, st = count.count_files(paths, k, t=t, dump=True, **kw)
    wk, wc, whist = dc.table_oracle(dc.sums(records), k, t)
    assert np.array_equal(dc.table_keys(tab), wk)
    assert np.array_equal(tab.counts, wc)
    assert np.array_equal(hist, whist) and hist[0] == 0
    assert st["windows"] == len(records) and st["bases"] == k * len(records)
    assert st["distinct"] == int(whist.sum()) and st["kept"] == len(wc) and st["used"] == 1
    return st


@pytest.mark.parametrize("t", [1, 4])
@pytest.mark.parametrize("k", [21, 32, 33, 64, 97, 128])
def test_counting_a_dump_gives_the_table_of_the_oracle(k, t, tmp_path):
    rng = random.Random(k)
    kmers = dc.random_kmers(k, 3000, seed=k)
    # a canonical dump of distinct k-mers
    uniq = [(dc.canonical(s), rng.choice([1, 2, 3, 5, 40, 32766, 32767, 32768, 70000])) for s in kmers]
    (tmp_path / "u.txt").write_bytes(dc.text(uniq))
    counted(tmp_path / "u.txt", k, t, uniq)
    # both strands (Jellyfish without -C), palindromes where k is even, repeated k-mers, sums of exactly 32767 and 32768,
    # two lines of 2^32 - 1 (which saturate and do not wrap), lower case, CRLF
    both = []
    for i, s in enumerate(kmers[:1500]):
        both.append((s, 1 + i % 7, " "))
        both.append((dc.revcomp(s).lower(), 2 + i % 5, "\t", "\r\n"))
    if k % 2 == 0:
        both += [(s, 3) for s in dc.palindromes(k, 50, seed=1)] * 2
    both += [(kmers[2000], 32766), (dc.revcomp(kmers[2000]), 1), (kmers[2001], 32766), (kmers[2001], 2),
             (kmers[2002], 4294967295), (dc.revcomp(kmers[2002]), 4294967295), (kmers[2003], 4294967295), (kmers[2003], 1),
             (kmers[2004], "9" * 20), (kmers[2005], 4294967296)]
    rng.shuffle(both)
    (tmp_path / "b.txt").write_bytes(dc.text(both))
    st = counted(tmp_path / "b.txt", k, t, both)
    d = dc.sums(both)
    assert d[dc.canonical(kmers[2000])] == 32767 and d[dc.canonical(kmers[2001])] == 32768
    assert st["distinct"] < len(both)


def test_a_run_across_workgroups_and_past_65535_and_a_k_mer_that_meets_itself_in_every_merge(tmp_path, monkeypatch):
    k = 31
    kmers = dc.random_kmers(k, 200, seed=8)
    one = [(kmers[0] if i % 3 else dc.revcomp(kmers[0]), 1) for i in range(70_000)]
    recs = one[:35_000] + [(s, 2) for s in kmers[1:]] + one[35_000:] + [(kmers[1], 32765)]
    (tmp_path / "r.txt").write_bytes(dc.text(recs))
    st = counted(tmp_path / "r.txt", k, 1, recs)
    assert st["batches"] == 1
    tab, hist, _ = count.count_files(tmp_path / "r.txt", k, t=30000, dump=True)
    assert tab.counts.tolist() == [32767, 32767] and hist[32767] == 2          # 70 000 clamps, 2 + 32765 is exactly 32767
    big = [(kmers[0], 4294967295)] * 3 + [(kmers[5], 65536)] * 65_536              # 65536 x 65536 is 2^32: a sum that wrapped would be 0
    (tmp_path / "s.txt").write_bytes(dc.text(big))
    counted(tmp_path / "s.txt", k, 1, big)
    # the same k-mer in every batch of 4096 text bytes: it meets itself in every merge
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", "4096")
    few = [(kmers[i % 50] if i % 2 else dc.revcomp(kmers[i % 50]), 1 + i % 3) for i in range(3000)] + [(s, 1) for s in kmers[50:]]
    (tmp_path / "m.txt").write_bytes(dc.text(few))
    st = counted(tmp_path / "m.txt", k, 1, few)
    assert st["batches"] >= len(dc.text(few)) // (4096 + k) > 20
    for t in (1, 4):
        counted(tmp_path / "m.txt", k, t, few)


def test_three_dumps_three_readers_any_order(tmp_path):
    k = 51
    kmers = dc.random_kmers(k, 4000, seed=12)
    parts = [[(s, 1 + (i + j) % 9) for i, s in enumerate(kmers[j * 1000: j * 1000 + 2000])] for j in range(3)]
    parts[1] = [(dc.revcomp(s), c) for s, c in parts[1]]
    paths = []
    for j, recs in enumerate(parts):
        paths.append(tmp_path / f"s{j}.txt")
        paths[-1].write_bytes(dc.text(recs, last_end="" if j == 1 else None))
    allrecs = parts[0] + parts[1] + parts[2]
    for t in (1, 4):
        for order, threads in (((0, 1, 2), 3), ((2, 0, 1), 1), ((1, 2, 0), 2)):
            counted([paths[i] for i in order], k, t, allrecs, threads=threads)


def test_compressed_dumps_give_the_table_of_the_plain_file(tmp_path):
    k = 31
    kmers = dc.random_kmers(k, 20_000, seed=21)
    recs = [(s, 1 + i % 50) for i, s in enumerate(kmers)]
    text = dc.text(recs)
    assert len(text) > 9 * 65280
    (tmp_path / "d.txt").write_bytes(text)
    (tmp_path / "d.txt.bgz").write_bytes(bz.bgzf(text))
    (tmp_path / "d.txt.gz").write_bytes(gc.gz(text))
    plain = count.count_files(tmp_path / "d.txt", k, t=2, dump=True)
    counted(tmp_path / "d.txt", k, 2, recs)
    for name, gz_on in (("d.txt.bgz", False), ("d.txt.gz", True), ("d.txt.bgz", True)):
        got = count.count_files(tmp_path / name, k, t=2, dump=True, gzip=gz_on)
        assert np.array_equal(got[0].packed, plain[0].packed) and np.array_equal(got[0].counts, plain[0].counts)
        assert np.array_equal(got[1], plain[1]) and got[2]["windows"] == len(recs)
        dk, dcn = same_records(tmp_path / name, k, gzip_on=True)
        hk, hc = count.dump_parse(tmp_path / "d.txt", k)
        assert sorted(zip(map(tuple, dk.tolist()), dcn.tolist())) == sorted(zip(map(tuple, hk.tolist()), hc.tolist()))
    with pytest.raises(count.CountError) as e:                      # plain gzip without the other option: refused as always
        count.count_files(tmp_path / "d.txt.gz", k, dump=True)
    assert e.value.code == -2 and "gzip compressed" in str(e.value)
    # compressed reads under the dump option: the reader thread says what the survey says of a plain file
    (tmp_path / "r.fq.gz").write_bytes(bz.bgzf(b"@r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n"))
    with pytest.raises(count.CountError) as e:
        count.count_files(tmp_path / "r.fq.gz", k, dump=True)
    assert e.value.code == -2 and "a call with the dump option reads dumps only" in str(e.value)
    # a bad line in a BGZF dump: the offset is that in the text
    cut = text.rfind(b"\n", 0, 400_000) + 1
    bad = text[:cut] + b"ACGT\n" + text[cut:]
    (tmp_path / "bad.bgz").write_bytes(bz.bgzf(bad))
    with pytest.raises(count.CountError) as e:
        count.count_files(tmp_path / "bad.bgz", k, dump=True)
    assert e.value.code == -4 and str(e.value).endswith(f"bad.bgz: dump line at offset {cut}: {dc.REASONS['bases'].format(k=k)}")


def test_reads_to_table_to_dump_to_table_and_to_the_plot(tmp_path):
    k, e = 21, 3
    reads = gc.het_fastq()
    (tmp_path / "r.fq").write_bytes(reads)
    tab, hist, st = count.count_files(tmp_path / "r.fq", k, t=1)
    keys = dc.table_keys(tab)
    kmers = [dc.unwords(r, k) for r in keys.tolist()]
    assert len(kmers) > 3000 and tab.counts.max() < 32767
    rng = random.Random(5)
    canon = [(s, int(c)) for s, c in zip(kmers, tab.counts)]
    split = []
    for s, c in canon:
        a = rng.randint(0, c)
        split += [(x, n) for x, n in ((s, a), (dc.revcomp(s), c - a)) if n]
    rng.shuffle(split)
    (tmp_path / "canon.txt").write_bytes(dc.text(canon))
    (tmp_path / "split.txt").write_bytes(dc.text(split, sep=" "))
    for name in ("canon.txt", "split.txt"):
        got, ghist, gst = count.count_files(tmp_path / name, k, t=1, dump=True)
        assert np.array_equal(got.packed, tab.packed) and np.array_equal(got.counts, tab.counts) and np.array_equal(ghist, hist)
    want_plot, want_hist, _ = count.reads_to_plot(tmp_path / "r.fq", k, 1, e)
    assert want_plot.sum() > 0
    for name in ("canon.txt", "split.txt"):
        plot, phist, _ = count.reads_to_plot(tmp_path / name, k, 1, e, dump=True)
        assert np.array_equal(plot, want_plot) and np.array_equal(phist, want_hist)
    # the executable: -d -e writes the .smu that it writes from the reads
    for args in (["-k21", "-t1", f"-e{e}", "-n", "-oreads", "r.fq"], ["-k21", "-t1", f"-e{e}", "-n", "-d", "-odump", "split.txt"]):
        r = subprocess.run([COUNT_BIN, *args], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert (tmp_path / "reads.smu").read_bytes() == (tmp_path / "dump.smu").read_bytes()
