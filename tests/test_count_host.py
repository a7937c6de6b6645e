"""The k-mer counter's host side, no GPU: the FASTA / FASTQ parser against a Python parser, the exported symbols against the
header, and the argument errors of the `smg_count` executable.  libsmg_count.so must load without a device."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from smudgeplot_amd import count

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
COUNT_LIB = os.path.join(ROOT, "smudgeplot_amd", "libsmg_count.so")


def py_parse(data: bytes) -> bytes:
    """the sequence of every record, line ends removed, one newline between two records"""
    if not data:
        return b""
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in data.split(b"\n")]
    if data.endswith(b"\n"):
        lines.pop()
    seqs = []
    if data[:1] == b">":
        for ln in lines:
            if ln[:1] == b">":
                seqs.append(b"")
            else:
                seqs[-1] += ln
    else:
        assert data[:1] == b"@"
        i = 0
        while i < len(lines):
            if lines[i] == b"":                      # blank line between records
                i += 1
                continue
            seqs.append(lines[i + 1] if i + 1 < len(lines) else b"")
            i += 4
    return b"\n".join(seqs)


CASES = {
    "fasta_multiline": b">r1 some text\nACGTAC\nGGTT\nA\n>r2\nTTTT\n",
    "fasta_crlf": b">r1\r\nACGT\r\nACGG\r\n>r2\r\nGG\r\n",
    "fasta_no_final_newline": b">r1\nACGT\nAC",
    "fasta_empty_record": b">a\n>b\nACGT\n>c\n",
    "fasta_lower_and_n": b">x\nacgtnnnnACGTNNacgt\nnnnn\n>y\nNNNN\n",
    "fastq_plain": b"@r1\nACGTACGT\n+\nIIIIIIII\n@r2\nGGGG\n+r2\nIIII\n",
    "fastq_quality_starts_with_at_and_gt": b"@r1\nACGT\n+\n@III\n@r2\nGGTT\n+\n>III\n@r3\nAAAA\n+\n@@@@\n",
    "fastq_crlf": b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nAC\r\n+\r\nII\r\n",
    "fastq_no_final_newline": b"@r1\nACGT\n+\nIIII\n@r2\nGG\n+\nII",
    "fastq_empty_record": b"@r1\n\n+\n\n@r2\nACGT\n+\nIIII\n",
    "fastq_lower_and_n": b"@r1\nacgtNNNNacgtn\n+\nIIIIIIIIIIIII\n",
    "empty_file": b"",
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parser_equals_the_python_parser(name, tmp_path):
    p = tmp_path / "in.txt"
    p.write_bytes(CASES[name])
    assert count.parse(p) == py_parse(CASES[name])


def test_parser_on_input_larger_than_its_read_buffer(tmp_path):
    """records and '\\r\\n' pairs that straddle the 4 MiB pieces the file is read in"""
    import numpy as np
    rng = np.random.default_rng(5)
    recs = []
    for i in range(9000):
        n = int(rng.integers(0, 2000))
        s = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), n))
        recs.append(b"@r%d\r\n" % i + s + b"\r\n+\r\n" + bytes(rng.choice(np.frombuffer(b"@>I#", np.uint8), n)) + b"\r\n")
    data = b"".join(recs)
    assert len(data) > 3 * (4 << 20)
    p = tmp_path / "big.fq"
    p.write_bytes(data)
    assert count.parse(p) == py_parse(data)
    lines = []
    for i in range(300):
        lines.append(b">c%d\r\n" % i)
        for _ in range(int(rng.integers(0, 700))):
            lines.append(bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 60)) + b"\r\n")
    data = b"".join(lines)
    assert len(data) > 4 << 20
    p = tmp_path / "big.fa"
    p.write_bytes(data)
    assert count.parse(p) == py_parse(data)


def test_gzip_and_unknown_input_are_refused_with_a_message(tmp_path):
    import gzip
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(gzip.compress(b"@r\nACGT\n+\nIIII\n"))
    with pytest.raises(count.CountError) as e:
        count.parse(p)
    assert e.value.code == -2 and "gzip" in str(e.value) and "not supported" in str(e.value)
    q = tmp_path / "reads.txt"
    q.write_bytes(b"ACGT\n")
    with pytest.raises(count.CountError) as e:
        count.parse(q)
    assert "neither FASTA nor FASTQ" in str(e.value)
    with pytest.raises(count.CountError) as e:
        count.parse(tmp_path / "absent.fa")
    assert "cannot open" in str(e.value)


def test_library_exports_what_the_header_declares():
    hdr = open(os.path.join(ROOT, "include", "smg_count.h")).read()
    declared = set(re.findall(r"\b(smg_count_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(count.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", COUNT_LIB], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r" T (smg_count_[a-z0-9_]+)$", out, flags=re.M))
    assert defined == declared
    assert "gfx950" in count.version()
    # the counter is a library of its own: nothing of it in the hetmers engine's ABI
    from smudgeplot_amd import engine
    assert not any(n.startswith("smg_count") for n in engine.EXPORTS)


def run(args, cwd):
    return subprocess.run([COUNT_BIN, *args], cwd=cwd, capture_output=True, text=True)


def test_smg_count_argument_errors_write_nothing(tmp_path):
    (tmp_path / "r.fa").write_bytes(b">a\nACGTACGTACGTACGTACGT\n")
    for args, msg in ((["-k12", "r.fa"], "K-mer length must be 13 .. 128 (12)"),
                      (["-k129", "r.fa"], "K-mer length must be 13 .. 128 (129)"),
                      ([], "Usage: smg_count"),
                      (["-k21"], "Usage: smg_count"),
                      (["-k21", "absent.fa"], "Cannot open absent.fa"),
                      (["-kx", "r.fa"], "argument is not an integer"),
                      (["-t0", "r.fa"], "must be positive"),
                      (["-z", "r.fa"], "-z is an illegal option")):
        r = run(args, tmp_path)
        assert r.returncode == 1, (args, r.stderr)
        assert msg in r.stderr, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["r.fa"], args
    os.chmod(tmp_path / "r.fa", 0)
    if not os.access(tmp_path / "r.fa", os.R_OK):          # (root reads anything)
        r = run(["-k21", "r.fa"], tmp_path)
        assert r.returncode == 1 and "Cannot open r.fa" in r.stderr
        assert sorted(os.listdir(tmp_path)) == ["r.fa"]


def test_smg_count_refuses_gzip_before_it_writes(tmp_path):
    import gzip
    (tmp_path / "r.fq.gz").write_bytes(gzip.compress(b"@r\nACGT\n+\nIIII\n"))
    r = run(["-k21", "-H", "r.fq.gz"], tmp_path)
    assert r.returncode == 1 and "gzip" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["r.fq.gz"]
