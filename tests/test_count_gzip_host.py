"""Plain gzip in front of the k-mer counter, without a GPU: the host twin of the device route (count.gzip_text_host: the same
block finder, marker decoder, chain, resolver and exact decoder as the kernels, run as one lane) against Python's gzip over the
streams of tests/gzip_craft.py at every span size, what its report says, the refusals with their offsets, and that nothing
changes without the opt-in.  (`make gzip_check` holds the same twin against zlib under the sanitizers over mutated files; it
takes a compiler and a minute and is run by hand; profiles/count_gzip.md keeps its output.)  The streams here are some 300 KB
at ordinary ratios; tests/test_count_gzip_seams_host.py holds the twin against files that reach the fixed sizes of the code --
the spans of a piece, the ring slots of a decode, the intervals and the text of one call -- and has the refusals of the resolver
and of a block above the text of one call."""
import gzip
import os
import re
import subprocess

import pytest

import gzip_craft as gc
from conftest import ROOT
from smudgeplot_amd import count

REFUSAL = "is gzip compressed: compressed input is not supported, decompress it first"


@pytest.fixture(scope="module")
def text():
    t = gc.fastq_text()
    assert 290_000 < len(t) < 320_000 and b"A" * 40_000 in t
    return t


@pytest.fixture(scope="module")
def files(text, tmp_path_factory):
    """name -> (path, text)"""
    d = tmp_path_factory.mktemp("gzip")
    out = {}
    for name, (data, want) in gc.streams(text).items():
        p = d / f"{name}.fq.gz"
        p.write_bytes(data)
        out[name] = (str(p), want)
    return out


NAMES = ["level1", "level6", "level9", "fixed", "stored", "huffman_only", "rle", "memlevel1", "sync_flush", "two_members", "fifty_members",
         "header_fields", "trailing_zeros", "far_match", "gzip_in_gzip"]


def test_the_binding_has_the_calls_and_the_field_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "smg_count.h")).read()
    assert {"smg_count_gzip_inflate", "smg_count_gzip_text_host", "smg_count_gzip_report"} <= set(count.EXPORTS)
    assert re.search(r"int32_t verbose;\s*int32_t gzip;[^}]*}\s*smg_count_opts;", hdr), "gzip is the trailing field of the options"
    assert [n for n, _ in count.Opts._fields_][-1] == "gzip"
    assert count.GZIP_SPAN == 256 << 10


@pytest.mark.parametrize("span", gc.SPANS)
@pytest.mark.parametrize("name", NAMES)
def test_the_twin_gives_the_text_of_gzip_at_every_span(name, span, files):
    path, want = files[name]
    assert set(files) == set(NAMES)
    got = count.gzip_text_host(path, span)
    assert got == want
    r = count.gzip_report(path)
    members = {"two_members": 2, "fifty_members": 50}.get(name, 1)
    # every byte of text comes from a linked or a repaired decode, and every member has at least one (its final block)
    assert r["members"] == members and r["text_bytes"] == len(want)
    assert r["linked"] >= 1 and r["linked"] + r["repaired"] >= members
    # the spans tile the file: a piece of 256 spans rounds up once, and trailing zeros (1000 bytes here) are no span
    size = os.path.getsize(path)
    assert abs(r["spans"] - -(-size // span)) <= 1 + size // (256 * span)


def test_small_blocks_link_most_spans(files):
    # memLevel 1: a block is 128 symbols, some hundred compressed bytes, so every span of 4 KiB begins several blocks and its
    # first one is found; the twin linked 20 of 20 spans here (the issue asks for one half)
    path, _ = files["memlevel1"]
    count.gzip_text_host(path, 4 << 10)
    r = count.gzip_report(path)
    print(r)
    assert r["spans"] >= 20 and 2 * r["linked"] >= r["spans"]


@pytest.mark.parametrize("span", [1 << 10, 4 << 10])
@pytest.mark.parametrize("name", ["stored", "fixed", "gzip_in_gzip"])
def test_what_is_no_dynamic_block_is_repaired(name, span, files):
    # stored and fixed blocks are no candidates (and the final block never is), and the dynamic block headers inside the stored
    # blocks of gzip_in_gzip are false ones: where the chain arrives no span is waiting, so the decode goes on from the known
    # end.  At these spans every one of the three streams has block boundaries in several spans.
    path, want = files[name]
    assert count.gzip_text_host(path, span) == want
    r = count.gzip_report(path)
    print(r)
    assert r["repaired"] >= 1


def test_the_report_is_of_the_last_call_and_the_span_is_checked(files, tmp_path):
    path, want = files["level6"]
    count.gzip_text_host(path, 4 << 10)
    assert count.gzip_report(path)["text_bytes"] == len(want)
    other = files["level1"][0]
    count.gzip_text_host(other, 4 << 10)
    with pytest.raises(count.CountError):
        count.gzip_report(path)
    for span in (1023, (1 << 20) + 1, -5):
        with pytest.raises(count.CountError) as e:
            count.gzip_text_host(path, span)
        assert e.value.code == -2 and "span" in str(e.value)
    plain = tmp_path / "reads.fq"
    plain.write_bytes(want)
    with pytest.raises(count.CountError) as e:
        count.gzip_text_host(str(plain), 0)
    assert e.value.code == -2 and "is not gzip" in str(e.value)


def test_the_span_hook_of_the_environment(files, monkeypatch):
    path, want = files["memlevel1"]
    monkeypatch.setenv("SMG_COUNT_GZIP_SPAN", "1024")
    assert count.gzip_text_host(path) == want
    assert count.gzip_report(path)["spans"] == -(-os.path.getsize(path) // 1024)
    monkeypatch.delenv("SMG_COUNT_GZIP_SPAN")
    assert count.gzip_text_host(path) == want
    assert count.gzip_report(path)["spans"] == 1


def test_bgzf_is_gzip_too(text, tmp_path):
    import bgzf_craft as bz
    p = tmp_path / "reads.fq.gz"
    p.write_bytes(bz.bgzf(text[:200_000]))
    assert count.gzip_text_host(str(p), 4 << 10) == text[:200_000]
    assert count.gzip_report(str(p))["members"] == 5


@pytest.mark.parametrize("span", [1 << 10, 64 << 10])
def test_every_refusal_names_its_offset(span, text, tmp_path):
    for name, (data, off, why) in gc.damaged(text).items():
        with pytest.raises(Exception):
            gzip.decompress(data)
        p = tmp_path / "bad.fq.gz"
        p.write_bytes(data)
        with pytest.raises(count.CountError) as e:
            count.gzip_text_host(str(p), span)
        msg = str(e.value)
        assert e.value.code == -4, (name, msg)
        if off is None:
            assert re.search(rf"{re.escape(str(p))}: deflate block at offset \d+: ", msg) and why in msg, (name, msg)
        else:
            assert f"{p}: gzip member at offset {off}: " in msg and why in msg, (name, msg)


# ---- nothing changes without the opt-in ---------------------------------------------------------------------------------

def test_without_the_option_gzip_is_refused_as_it_always_was(files):
    path, _ = files["level6"]
    for call in (lambda: count.count_files(path, 21), lambda: count.count_files([path], 21, gzip=False), lambda: count.parse(path),
                 lambda: count.bgzf_scan(path)):
        with pytest.raises(count.CountError) as e:
            call()
        assert e.value.code == -2 and str(e.value).endswith(f"{path} {REFUSAL}"), str(e.value)


def test_smg_count_without_g_behaves_as_before(text, tmp_path):
    (tmp_path / "r.fq.gz").write_bytes(gzip.compress(text[:5000]))
    r = subprocess.run([count.BIN_PATH, "-k21", "-H", "r.fq.gz"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and f"r.fq.gz {REFUSAL}" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["r.fq.gz"]
    r = subprocess.run([count.BIN_PATH, "-z", "r.fq.gz"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "-z is an illegal option" in r.stderr
    r = subprocess.run([count.BIN_PATH], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "[-g]" in r.stderr and "-g: read plain gzip" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["r.fq.gz"]
