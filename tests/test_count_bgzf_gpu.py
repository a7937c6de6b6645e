"""The BGZF route of the k-mer counter on the GPU: the inflate kernel byte by byte through count.bgzf_inflate (the oracle is
the text a fixture was made from), counting from BGZF files against the plain run and tests/count_oracle.py, and the
refusals, whose streams tests/test_count_bgzf_host.py holds against zlib and `make inflate_check` has passed on the CPU."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_craft as bz
import count_oracle
from smudgeplot_amd import count

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 257, 258, 259, 32767, 32768, 32769, 65280, 65535, 65536]
KINDS = {"stored": (0, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "dynamic1": (1, zlib.Z_DEFAULT_STRATEGY),
         "dynamic6": (6, zlib.Z_DEFAULT_STRATEGY), "dynamic9": (9, zlib.Z_DEFAULT_STRATEGY), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY),
         "rle": (6, zlib.Z_RLE)}


def fastq_like(rng, n):
    reads = []
    size = 0
    while size < n:
        m = int(rng.integers(30, 151))
        r = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), m, p=[0.2475] * 4 + [0.01]))
        q = bytes(rng.choice(np.frombuffer(b"I9#F,", np.uint8), m, p=[0.8, 0.05, 0.05, 0.05, 0.05]))
        reads.append(b"@read%d\n%s\n+\n%s\n" % (len(reads), r, q))
        size += len(reads[-1])
    return b"".join(reads)[:n]


@pytest.fixture(scope="module")
def text():
    return fastq_like(np.random.default_rng(7), 70000)


def inflate(tmp_path, data, name="x.gz"):
    p = tmp_path / name
    p.write_bytes(data)
    return count.bgzf_inflate(str(p))[0]


# ---- 1. block kinds and sizes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(KINDS))
def test_block_kinds_at_every_size(kind, text, tmp_path):
    level, strategy = KINDS[kind]
    members, want = [], []
    for n in SIZES:
        piece = text[1000:1000 + n]
        try:
            members.append(bz.member(bz.deflate(piece, level, strategy), piece))
        except bz.BsizeError:                                   # (level 0 cannot hold it)
            assert kind == "stored" and n > 65280
            continue
        want.append(piece)
    assert len(want) >= 11
    assert inflate(tmp_path, b"".join(members)) == b"".join(want)


@pytest.mark.parametrize("level", [1, 6])
def test_several_deflate_blocks_in_one_member(level, text, tmp_path):
    members = []
    for n, at in ((65280, 30000), (65280, 0), (40000, 40000), (3, 1)):
        members.append(bz.member(bz.deflate(text[:n], level, full_flush_at=at), text[:n]))
    w = bz.Bits()                                                # stored, fixed, stored and empty, dynamic by zlib is above
    bz.stored_block(w, text[:70], final=False)
    bz.fixed_block(w, list(text[70:90]) + [(20, 20), (258, 1)], final=False)
    bz.stored_block(w, b"", final=False)
    bz.stored_block(w, text[:5])
    mixed = text[:70] + bz.expand(list(text[70:90]) + [(20, 20), (258, 1)]) + text[:5]
    members.append(bz.member(w.done(), mixed))
    assert inflate(tmp_path, b"".join(members)) == text[:65280] * 2 + text[:40000] + text[:3] + mixed


# ---- 2. matches ---------------------------------------------------------------------------------------------------------

def test_every_match_length_at_every_distance_and_across_the_window_seams(tmp_path):
    made = bz.match_members()
    names = sorted(made)
    got = inflate(tmp_path, b"".join(bz.member(*made[n]) for n in names))
    assert len(got) == 65536 * len(names)
    for i, n in enumerate(names):
        mine, want = got[65536 * i:65536 * (i + 1)], made[n][1]
        if mine != want:
            at = next(j for j in range(65536) if mine[j] != want[j])
            raise AssertionError(f"member {n}: first difference at text offset {at}")


# ---- 3. dynamic blocks by hand ------------------------------------------------------------------------------------------

def test_hand_made_dynamic_blocks(tmp_path):
    made = bz.dynamic_members()
    for name, (payload, want) in made.items():
        assert inflate(tmp_path, bz.member(payload, want) + bz.EOF_MARKER, name + ".gz") == want, name


# ---- 4. scheduling ------------------------------------------------------------------------------------------------------

def test_more_blocks_than_waves(text, tmp_path):
    rng = np.random.default_rng(11)
    sizes = [int(x) for x in rng.integers(1, 41, 5000)]
    want = (text * 2)[:sum(sizes)]
    p = tmp_path / "small.gz"
    p.write_bytes(bz.bgzf(want, level=6, sizes=sizes))
    assert count.bgzf_scan(str(p)) == {"blocks": 5001, "text_bytes": len(want)}
    got, ms = count.bgzf_inflate(str(p))
    assert got == want and ms > 0


def test_a_file_of_more_than_two_chunks(text, tmp_path):
    rng = np.random.default_rng(12)
    noise = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    members, want, size, i = [], [], 0, 0
    packed = [bz.member(bz.deflate(text[j:j + 65000], 1), text[j:j + 65000]) for j in range(0, 5000, 1000)]
    while size <= 2 * count.BGZF_CHUNK + (1 << 20):
        j = (i * 7919) % ((1 << 20) - 65280)
        piece = noise[j:j + 65280 - i % 3]                       # (three lengths, so that the seams between launches move)
        members += [bz.member(bz.deflate(piece, 0), piece), packed[i % 5]]
        want += [piece, text[(i % 5) * 1000:(i % 5) * 1000 + 65000]]
        size += len(members[-1]) + len(members[-2])
        i += 1
    p = tmp_path / "big.gz"
    p.write_bytes(b"".join(members))
    assert os.path.getsize(p) > 2 * count.BGZF_CHUNK
    got, _ = count.bgzf_inflate(str(p))
    want = b"".join(want)
    assert len(got) == len(want) and got == want


# ---- 5. counting --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reads():
    rng = np.random.default_rng(5)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)
    other = genome.copy()                                        # a second haplotype: a substitution every 97 bases
    other[50::97] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), other[50::97])]
    out = []
    for i in range(700):
        a = int(rng.integers(0, 3000 - 160))
        r = bytes((genome if i % 4 < 2 else other)[a:a + int(rng.integers(70, 160))])
        if i % 2:
            r = r.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
        if i % 50 == 0:
            r = r[:30] + b"N" + r[31:]
        out.append(r)
    return out


@pytest.fixture(scope="module")
def inputs(reads, tmp_path_factory):
    """the same reads as plain FASTQ, as BGZF FASTQ with CRLF and as BGZF multi-line FASTA, in members whose seams cut
    records, lines and CR LF pairs (sizes that share no factor with the line lengths)"""
    d = tmp_path_factory.mktemp("bgzf_counting")
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    fa = b"".join(b">s%d\r\n" % i + b"".join(r[j:j + 60] + b"\r\n" for j in range(0, len(r), 60)) for i, r in enumerate(reads))
    crlf = fq.replace(b"\n", b"\r\n")
    cr = [i for i in range(len(crlf) - 1) if crlf[i:i + 2] == b"\r\n"]
    sizes = [cr[5] + 1, cr[9] - cr[5], 997, 1, 2, 4099, 65280]     # the first two seams fall between a CR and its LF
    files = {"plain": fq, "fq_crlf": bz.bgzf(crlf, level=6, sizes=sizes), "fa_multi": bz.bgzf(fa, level=1, sizes=[1009, 3, 65536], eof=False)}
    paths = {}
    for name, data in files.items():
        paths[name] = str(d / (name + (".fq" if name == "plain" else ".gz")))
        open(paths[name], "wb").write(data)
    assert crlf[sizes[0] - 1:sizes[0] + 1] == b"\r\n" and crlf[sizes[0] + sizes[1] - 1:sizes[0] + sizes[1] + 1] == b"\r\n"
    return paths


_ORACLE = {}


def oracle(reads, k, t, copies=1):
    if (k, t, copies) not in _ORACLE:
        keys, cnts, _ = count_oracle.kmer_counts(count_oracle.pad_reads(reads * copies), k)
        _ORACLE[(k, t, copies)] = count_oracle.table(keys, cnts, k, t)
    return _ORACLE[(k, t, copies)]


def same(got, want_packed, want_counts, want_hist):
    table, hist, _ = got
    assert np.array_equal(table.packed, want_packed) and np.array_equal(table.counts, want_counts) and np.array_equal(hist, want_hist)


@pytest.mark.parametrize("t", [1, 4])
@pytest.mark.parametrize("k", [21, 65])
def test_counting_from_bgzf_equals_the_plain_run_and_the_oracle(k, t, reads, inputs):
    plain = count.count_files(inputs["plain"], k, t=t, threads=1)
    same(plain, *oracle(reads, k, t))
    for name in ("fq_crlf", "fa_multi"):
        got = count.count_files(inputs[name], k, t=t, threads=1)
        same(got, plain[0].packed, plain[0].counts, plain[1])
        assert got[2]["bases"] == plain[2]["bases"]


@pytest.mark.parametrize("threads", [1, 3])
def test_a_mixed_list_of_plain_and_bgzf_files(threads, reads, inputs):
    k, t = 21, 1
    paths = [inputs["fq_crlf"], inputs["plain"], inputs["fa_multi"], inputs["plain"], inputs["fq_crlf"]]
    same(count.count_files(paths, k, t=t, threads=threads), *oracle(reads, k, t, copies=5))
    same(count.count_files(paths[::-1], 65, t=4, threads=threads), *oracle(reads, 65, 4, copies=5))


def test_partitioned_counting_from_bgzf(reads, inputs):
    got = count.count_files([inputs["fq_crlf"], inputs["fa_multi"]], 21, t=1, threads=3, partitions=3)
    assert got[2]["used"] == 3
    same(got, *oracle(reads, 21, 1, copies=2))


def test_the_executable_reads_bgzf_and_names_its_output_after_the_reads(reads, inputs, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    (a / "reads.fq").write_bytes(open(inputs["plain"], "rb").read())
    (b / "reads.fq.gz").write_bytes(open(inputs["fq_crlf"], "rb").read())
    for d, name in ((a, "reads.fq"), (b, "reads.fq.gz")):
        r = subprocess.run([count.BIN_PATH, "-k21", "-t1", "-H", "-v", name], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        if name.endswith(".gz"):
            scan = count.bgzf_scan(inputs["fq_crlf"])
            assert f"reads.fq.gz: BGZF, {scan['blocks']} blocks, {scan['text_bytes']} text bytes, inflated on the device" in r.stderr
    for name in ("reads.ktab", ".reads.ktab.1", "reads.hist.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    for d, name in ((a, "reads.fq"), (b, "reads.fq.gz")):
        r = subprocess.run([count.BIN_PATH, "-k21", "-t2", "-e2", "-n", name], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert (a / "reads.smu").read_bytes() == (b / "reads.smu").read_bytes() and (a / "reads.smu").stat().st_size > 0


# ---- 6. refusals --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(bz.invalid_members()))
def test_a_bad_member_is_refused_with_its_offset_and_reason(name, reads, inputs, tmp_path):
    payload, isize, crc, reason = bz.invalid_members()[name]
    good = bz.member(bz.deflate(bz.TEXT), bz.TEXT)
    d = tmp_path / "run"
    d.mkdir()
    path = d / "bad.fq.gz"
    path.write_bytes(good + good + bz.member(payload, isize=isize, crc=crc) + good + bz.EOF_MARKER)
    for call in (lambda: count.bgzf_inflate(str(path)), lambda: count.count_files([inputs["plain"], str(path)], 21, t=1, threads=2)):
        with pytest.raises(count.CountError) as e:
            call()
        assert e.value.code == -4, str(e.value)
        assert f"{path}: BGZF block at offset {2 * len(good)}: " in str(e.value) and reason in str(e.value), str(e.value)
    r = subprocess.run([count.BIN_PATH, "-k21", "-t1", "-H", "bad.fq.gz"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 1 and f"BGZF block at offset {2 * len(good)}" in r.stderr
    assert sorted(os.listdir(d)) == ["bad.fq.gz"]
    same(count.count_files(inputs["fa_multi"], 21, t=1, threads=1), *oracle(reads, 21, 1))      # a valid run afterwards, same process
