"""Plain gzip where the fixed sizes of csrc/smg_gzip.hpp are reached, without a GPU: the host twin (count.gzip_text_host) against
Python's gzip over gc.seam_streams(), and what its report must say for the file to have reached the size it is made for --
the 256 spans of a piece and every kind of byte a piece can end in, the 8 ring slots of a speculative decode and the 64 of a
repair, the 4096 intervals and the 64 MiB of text of one call of the second pass -- and the one refusal only the resolver can
give, a distance that reaches in front of its member.  tests/test_count_gzip_seams_gpu.py holds the kernels against the same
files and against these reports; the slabs of windows exist on the device only."""
import os

import pytest

import gzip_craft as gc
from smudgeplot_amd import count

KIB = gc.KIB
CHECK_1K = 16 * KIB                                              # text between two checkpoints at a span of 1 KiB: 16 spans' worth
CHECK_DEFAULT = 256 * KIB                                        # and at the default span
QUOTA, REPAIR_QUOTA = 8, 64                                      # ring slots of a speculative decode and of a repair


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, text)"""
    d = tmp_path_factory.mktemp("gzip_seams")
    out = {}
    for i, (name, (data, want)) in enumerate(gc.seam_streams().items()):
        p = d / f"s{i}.fq.gz"
        p.write_bytes(data)
        out[name] = (str(p), want)
    return out


def twin(path, want, span):
    got = count.gzip_text_host(path, span)
    assert len(got) == len(want) and got == want
    r = count.gzip_report(path)
    print(os.path.getsize(path), span, r)
    assert r["text_bytes"] == len(want)
    return r


def test_the_helper_gives_the_streams_and_the_seams_the_tests_name():
    assert set(gc.seam_streams()) == set(gc.SEAM_SPANS)
    assert len(gc.seam_header()) == 54
    assert sorted(gc.seam_deltas().values()) == [-4, 0, 1, 5, 20, 45, 54, 60, 200]
    reads = gc.np_fastq(50_000, 1)
    assert 50_000 <= len(reads) < 50_400 and reads.count(b"\n") % 4 == 0 and reads.startswith(b"@r0\n") and reads.endswith(b"\n")
    assert gc.np_fastq(50_000, 1) == reads != gc.np_fastq(50_000, 2)


def test_more_intervals_than_one_launch_of_the_exact_decoder_holds(files, tmp_path):
    # Every member is one decode at least, and every decode that is accepted begins a restart interval: points >= linked +
    # repaired, and equal where no decode wrote a checkpoint.  The members of the prefix hold 70 bytes of text each, far below
    # the 16 KiB between two checkpoints, so its count is exact: below 4096.  With the large member it is above: interval
    # number 4096, where the second launch begins, lies inside that member, and its CRC-32 is joined over the two launches.
    prefix, big, tail = gc.many_members_parts()
    path, want = files["many_members"]
    a, b = tmp_path / "prefix.fq.gz", tmp_path / "prefix_big.fq.gz"
    a.write_bytes(prefix[0])
    b.write_bytes(prefix[0] + big[0])
    ra = twin(str(a), prefix[1], KIB)
    rb = twin(str(b), prefix[1] + big[1], KIB)
    r = twin(path, want, KIB)
    na, nb, nt = prefix[2], big[2], tail[2]
    assert (na, nb, nt) == (4050, 1, 400) and gc.gz(b"", 6) in tail[0] and want == prefix[1] + big[1] + tail[1]
    assert (ra["members"], rb["members"], r["members"]) == (na, na + 1, na + 1 + nt)
    points = [x["linked"] + x["repaired"] for x in (ra, rb, r)]
    assert points[0] == na < gc.MAX_EXACT < points[1] and points[2] > gc.MAX_EXACT + 300
    assert points[2] > 8 * 512                                  # (one window each: more than eight slabs of 512 on the device)
    assert r["repaired"] >= na + nt - r["spans"]                # a final block is no candidate: but for the first of a piece, a repair each


def test_a_file_of_two_pieces_whose_first_launch_is_full(files):
    path, want = files["two_pieces"]
    size = os.path.getsize(path)
    assert gc.PIECE_1K < size <= 512 * KIB                      # 256 tasks in the first launch, and a second piece
    r = twin(path, want, KIB)
    assert r["members"] == 1 and r["spans"] > 256 and r["spans"] >= size // KIB
    assert 2 * r["linked"] >= r["spans"]                        # the blocks of memLevel 1 are found, beyond the seam too


@pytest.mark.parametrize("name", list(gc.seam_deltas()))
def test_a_piece_ends_in_every_kind_of_byte(name, files):
    delta = gc.seam_deltas()[name]
    path, want = files[f"piece_seam: {name}"]
    data = open(path, "rb").read()
    second = data.index(gc.seam_header(), 1000)
    hlen = len(gc.seam_header())
    assert second == gc.PIECE_1K - delta and data.count(gc.seam_header()) == 1
    at = gc.PIECE_1K - second                                   # the first byte of the second piece, counted from the second member
    if "trailer" in name:
        assert -8 < at < 0
    elif "ends with the piece" in name:
        assert at == (0 if "member" in name else hlen)
    elif "fixed" in name:
        assert 0 < at < 10
    elif "FNAME" in name:
        assert 10 < at < 10 + len(gc.SEAM_NAME)
    elif "FCOMMENT" in name:
        assert 11 + len(gc.SEAM_NAME) < at < hlen - 1
    else:
        assert hlen < at < hlen + 8 if "header" in name else at > hlen + 100
    r = twin(path, want, KIB)
    assert r["members"] == 2 and r["spans"] >= len(data) // KIB


def test_a_speculative_decode_runs_out_of_its_ring_slots(files):
    # blocks of 128 matches, 33 KB of text: every block boundary is a checkpoint, a decode has 8 slots and every span holds
    # more than 8 * 16 KiB of text, so no speculative decode reaches the end of its span: a repair goes on from where it stopped
    path, want = files["runs_small_blocks"]
    r = twin(path, want, KIB)
    assert r["members"] == 1 and r["spans"] == -(-os.path.getsize(path) // KIB)
    assert r["linked"] == r["repaired"] == r["spans"]
    assert r["text_bytes"] / r["spans"] > QUOTA * CHECK_1K


def test_a_repair_runs_out_of_its_ring_slots(files):
    # fixed blocks are no candidates: nothing but the quota or the end of the member ends a repair
    path, want = files["runs_fixed"]
    r = twin(path, want, KIB)
    assert r["members"] == 1 and r["repaired"] >= 2
    assert r["text_bytes"] > r["repaired"] * (REPAIR_QUOTA - 1) * CHECK_1K / 2


def test_every_decode_uses_all_its_ring_slots_and_no_more(files):
    # Fixed blocks whose every boundary is a checkpoint, the first eight of them in the first span: a decode of n slots writes
    # n - 1 checkpoints and ends at the boundary of the n-th.  8 + 3 * 64 blocks are one speculative decode and three repairs,
    # the last of which ends with the final block; a decode that keeps one slot too many free needs a fourth.
    path, want = files["full_slots"]
    assert len(want) == (QUOTA + 3 * REPAIR_QUOTA) * 16518
    r = twin(path, want, KIB)
    assert (r["members"], r["linked"], r["repaired"]) == (1, 1, 3)


@pytest.mark.parametrize("span", gc.SEAM_SPANS["text_cap"])
def test_more_text_than_one_call_of_the_second_pass_holds(span, files):
    path, want = files["text_cap"]
    assert len(want) > gc.TEXT_CAP
    r = twin(path, want, span)
    assert r["members"] == 1
    if span == 0:                                               # one span: one speculative decode, and repairs that end on their quota
        assert r["spans"] == 1 and r["linked"] == 1 and r["repaired"] >= 2
        assert r["text_bytes"] > r["repaired"] * (REPAIR_QUOTA - 1) * CHECK_DEFAULT / 2
    else:
        assert r["spans"] == -(-os.path.getsize(path) // KIB) and r["repaired"] >= 2


@pytest.mark.parametrize("span", [KIB, 64 * KIB])
def test_a_distance_in_front_of_the_member_is_refused_by_the_resolver(span, tmp_path):
    damaged = gc.damaged_seams(gc.fastq_text(70_000, 1000))
    assert len(damaged) == 4 and sorted(off > 0 for _, off, _ in damaged.values()) == [False, False, True, True]
    for name, (data, off, why) in damaged.items():
        p = tmp_path / "bad.fq.gz"
        p.write_bytes(data)
        with pytest.raises(count.CountError) as e:
            count.gzip_text_host(str(p), span)
        assert e.value.code == -4 and str(e.value).endswith(f"{p}: gzip member at offset {off}: {why}"), (name, str(e.value))


def test_a_block_above_the_text_of_one_call_is_refused(tmp_path):
    data, text = gc.one_block_above_the_text_of_a_call()
    p = tmp_path / "block.fq.gz"
    p.write_bytes(data)
    with pytest.raises(count.CountError) as e:
        count.gzip_text_host(str(p), KIB)
    msg = str(e.value)
    assert e.value.code == -2 and f"{p}: the deflate block at offset 10 takes " in msg and f"inflates to {len(text)}, above the " in msg, msg
    assert msg.endswith("of one call: decompress the file first")
