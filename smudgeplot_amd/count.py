"""ctypes binding of the k-mer counter (include/smg_count.h, libsmg_count.so, built in-tree).

Reads in, canonical FastK-style k-mer table out: the step in front of `hetmers`.  There is no CPU
fallback: the counting calls raise `CountError` without a HIP device; `parse`, `bgzf_scan` and `bam_text` need none.
The input files are FASTA / FASTQ, plain or block-gzipped (BGZF, what `bgzip` writes); the members of a BGZF file are
inflated on the device.  Any other gzip file is refused -- that refusal is a tested contract, so reading plain gzip (what
`gzip`, `pigz` and a sequencer write) is opt-in: `count_files(..., gzip=True)` inflates such files on the device in parallel
(block finder, decode with an unknown window, chained spans, an exact second pass; csrc/smg_gzip.hpp) and changes nothing for
the plain, BGZF and BAM files of the same call.  Unaligned BAM (PacBio HiFi reads: a BGZF file whose text begins
BAM\\1) is read too: its records are framed on the host and their 4-bit sequences unpacked on the device; its primary
records (FLAG without 0x100 and 0x800) give the stream of a FASTA file of the same reads.  A BAM file is bounded by its text
like any BGZF file, 1.5 times its bases or more, so it may be counted by key range where one pass would have done, with the
same result.

K-mers that another tool has counted already are read too, again opt-in (`count_files(..., dump=True)`): the text dumps of
`kmc_dump`, `jellyfish dump -c` and `meryl print`, one line `<k-mer><space or tab><count>` per k-mer, plain, BGZF or (with
gzip=True) plain gzip.  With the option every file of the call is a dump; the lines are decoded on the device, every line adds
its count to the smaller of its k-mer and its reverse complement, and the sums saturate.  `dump_parse` is the host twin of
that decoder, `dump_records` its records as the kernel emits them.
`smg_count_opts` grew by one trailing field for it: `Opts` is the struct up to `gzip`, as it was, and `DumpOpts(Opts)` the whole
struct, which is what this module hands to the library.

An input may be a stream: the path "-" is standard input (at most once per call), and a path that is not a regular file (a
FIFO, /dev/stdin, /dev/fd/N) is opened once and read forward only, told by its first bytes as a file is.  `count_files`,
`reads_to_plot`, `parse` and `dump_parse` take such paths; plain gzip on a stream is refused with or without gzip=True, and the
calls that read a file twice (`bgzf_scan`, `bgzf_inflate`, `bam_strip`, `gzip_inflate`, `gzip_text_host`) refuse a stream.  A
call with a stream has no bound: `stream_plan` is its plan, and the result is that of the same bytes read from a file.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import ktab

MIN_KMER, MAX_KMER, MAX_COUNT, HIST, BINS = 13, 128, 32767, 32768, 4096
FINE_BINS = 1 << 24                       # the ends of a range are values of the leading 24 bits where a bin was split
BGZF_CHUNK = 16 << 20                     # compressed bytes of a BGZF file that one launch of the inflate kernel takes
BAM_TILE = 4096                           # stripped bytes of a BAM file that one workgroup of the unpack kernel writes
DUMP_LINE = 151                           # the longest legal line of a k-mer dump: 128 bases, a separator, 20 digits, \r\n
GZIP_SPAN = 256 << 10                     # compressed bytes of a span of a plain gzip file (1 KiB .. 1 MiB can be asked for)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsmg_count.so")
BIN_PATH = os.path.join(_HERE, "bin", "smg_count")

EXPORTS = ["smg_count_files", "smg_count_bases", "smg_count_files_parts", "smg_count_bases_parts", "smg_count_plan",
           "smg_count_plan_fine", "smg_count_parse", "smg_count_free", "smg_count_version",
           "smg_count_files_device", "smg_count_bases_device", "smg_count_device_free", "smg_count_memory_plan",
           "smg_count_bgzf_scan", "smg_count_bgzf_inflate", "smg_count_bam_text", "smg_count_bam_strip", "smg_count_bam_report",
           "smg_count_gzip_inflate", "smg_count_gzip_text_host", "smg_count_gzip_report",
           "smg_count_dump_parse", "smg_count_dump_records", "smg_count_stream_plan"]


class CountError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"smg_count error {code}: {msg}")
        self.code = code


class Opts(C.Structure):
    _fields_ = [("kmer", C.c_int32), ("minval", C.c_int32), ("device", C.c_int32),
                ("host_threads", C.c_int32), ("verbose", C.c_int32), ("gzip", C.c_int32)]


class DumpOpts(Opts):
    """The whole smg_count_opts: the fields of Opts and the one the struct grew by behind them.  This is what every call of
    this module hands to the library, which reads all seven fields; Opts alone is the struct as it was before `dump`."""
    _fields_ = [("dump", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("bases", C.c_int64), ("windows", C.c_int64), ("distinct", C.c_int64), ("kept", C.c_int64),
                ("batches", C.c_int64), ("ms_read", C.c_double), ("ms_extract", C.c_double), ("ms_sort", C.c_double),
                ("ms_reduce", C.c_double), ("ms_finish", C.c_double), ("ms_wall", C.c_double)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Parts(C.Structure):
    _fields_ = [("partitions", C.c_int32), ("max_entries", C.c_int64), ("used", C.c_int32), ("store_bytes", C.c_int64),
                ("ms_pack", C.c_double), ("ms_plan", C.c_double), ("split", C.c_int32)]


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CountError(-1, f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
    from .engine import _share_torch_hip_runtime      # one HIP runtime per process, torch's if torch is installed
    _share_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    tail = [C.POINTER(DumpOpts), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int), vp,
            C.POINTER(Stats), C.c_char_p, C.c_size_t]
    lib.smg_count_files.argtypes = [C.POINTER(C.c_char_p), C.c_int] + tail
    lib.smg_count_files.restype = C.c_int
    lib.smg_count_bases.argtypes = [vp, C.c_int64] + tail
    lib.smg_count_bases.restype = C.c_int
    ptail = [tail[0], C.POINTER(Parts)] + tail[1:]
    lib.smg_count_files_parts.argtypes = [C.POINTER(C.c_char_p), C.c_int] + ptail
    lib.smg_count_files_parts.restype = C.c_int
    lib.smg_count_bases_parts.argtypes = [vp, C.c_int64] + ptail
    lib.smg_count_bases_parts.restype = C.c_int
    lib.smg_count_files_device.argtypes = [C.POINTER(C.c_char_p), C.c_int] + ptail
    lib.smg_count_files_device.restype = C.c_int
    lib.smg_count_bases_device.argtypes = [vp, C.c_int64] + ptail
    lib.smg_count_bases_device.restype = C.c_int
    lib.smg_count_device_free.argtypes = [vp]
    lib.smg_count_device_free.restype = None
    lib.smg_count_plan.argtypes = [vp, C.c_int64, C.c_int32, vp, C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    lib.smg_count_plan.restype = C.c_int
    lib.smg_count_plan_fine.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    lib.smg_count_plan_fine.restype = C.c_int
    lib.smg_count_memory_plan.argtypes = [C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
    lib.smg_count_memory_plan.restype = C.c_int
    lib.smg_count_stream_plan.argtypes = [C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
    lib.smg_count_stream_plan.restype = C.c_int
    lib.smg_count_parse.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
    lib.smg_count_parse.restype = C.c_int
    lib.smg_count_bgzf_scan.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
    lib.smg_count_bgzf_scan.restype = C.c_int
    lib.smg_count_bgzf_inflate.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_char_p,
                                           C.c_size_t]
    lib.smg_count_bgzf_inflate.restype = C.c_int
    lib.smg_count_bam_text.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
    lib.smg_count_bam_text.restype = C.c_int
    lib.smg_count_bam_strip.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
    lib.smg_count_bam_strip.restype = C.c_int
    lib.smg_count_bam_report.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.smg_count_bam_report.restype = C.c_int
    lib.smg_count_gzip_inflate.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                           C.c_char_p, C.c_size_t]
    lib.smg_count_gzip_inflate.restype = C.c_int
    lib.smg_count_gzip_text_host.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
    lib.smg_count_gzip_text_host.restype = C.c_int
    lib.smg_count_gzip_report.argtypes = [C.c_char_p] + [C.POINTER(C.c_int64)] * 5 + [C.POINTER(C.c_double)]
    lib.smg_count_gzip_report.restype = C.c_int
    lib.smg_count_dump_parse.argtypes = [C.c_char_p, C.c_int32, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                         C.c_char_p, C.c_size_t]
    lib.smg_count_dump_parse.restype = C.c_int
    lib.smg_count_dump_records.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
    lib.smg_count_dump_records.restype = C.c_int
    lib.smg_count_free.argtypes = [vp]
    lib.smg_count_free.restype = None
    lib.smg_count_version.restype = C.c_char_p
    _lib = lib
    return lib


def version() -> str:
    return load_library().smg_count_version().decode()


def keys_to_packed(keys: np.ndarray, k: int) -> np.ndarray:
    """[N,W] uint64 left-aligned words -> [N,kbyte] uint8 packed (the layout of ktab.KTable.packed)."""
    n = keys.shape[0]
    kb = ktab.kbyte_of(k)
    return np.ascontiguousarray(keys.astype(">u8").view(np.uint8).reshape(n, 8 * keys.shape[1])[:, :kb])


def _table(k, t, keys, counts):
    packed = keys_to_packed(keys, k)
    pre = np.zeros(len(counts), dtype=np.int64)
    for j in range(3):
        pre = (pre << 8) | packed[:, j].astype(np.int64)
    index = np.cumsum(np.bincount(pre, minlength=1 << 24)).astype(np.int64)
    return ktab.KTable(k, 3, 1, t, packed, counts, index, np.array([len(counts)], np.int64))


def _run(call, k, t, device, threads, partitions, max_entries, gzip=False, dump=False):
    lib = load_library()
    opts = DumpOpts(int(k), int(t), int(device), int(threads), 0, int(bool(gzip)), int(bool(dump)))
    parts = Parts(int(partitions), int(max_entries), 0, 0, 0.0, 0.0)
    keys, cnt = C.c_void_p(), C.c_void_p()
    nels, words = C.c_int64(0), C.c_int(0)
    hist = np.zeros(HIST, dtype=np.uint64)
    st = Stats()
    err = C.create_string_buffer(1024)
    rc = call(lib, C.byref(opts), C.byref(parts), C.byref(keys), C.byref(cnt), C.byref(nels), C.byref(words),
              hist.ctypes.data_as(C.c_void_p), C.byref(st), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        n, w = nels.value, words.value
        k64 = np.ctypeslib.as_array(C.cast(keys, C.POINTER(C.c_uint64)), shape=(max(n, 1) * w,))[: n * w].copy().reshape(n, w)
        c16 = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint16)), shape=(max(n, 1),))[:n].copy()
    finally:
        lib.smg_count_free(keys)
        lib.smg_count_free(cnt)
    stats = st.asdict()
    stats.update(used=parts.used, store_bytes=parts.store_bytes, ms_pack=parts.ms_pack, ms_plan=parts.ms_plan, split=parts.split)
    return _table(int(k), int(t), k64, c16), hist, stats


def count_files(paths, k, t=4, device=0, threads=4, partitions=0, max_entries=0, gzip=False, dump=False):
    """-> (ktab.KTable of the canonical k-mers with count >= t, hist uint64[32768], stats dict)

    partitions: 0 lets the library count by key range where one pass is not guaranteed to fit, 1 is one pass,
    2 .. 4096 that many ranges; max_entries (test hook) plans as if one merge held only that many entries.
    The stats carry `used` (ranges), `store_bytes`, `ms_pack` and `ms_plan` of a partitioned run, and `split`: the bins of
    the leading 12 bits that held more windows than one merge and were split on their next 12 bits (automatic mode only).
    gzip: read plain gzip files too (off: they are refused, as always); gzip_report says what was read of each.
    dump: every file is a k-mer dump (see the top of this module); partitions must then be 0 or 1, stats["windows"] is the
    number of lines and stats["bases"] k times that."""
    paths = [os.fsencode(p) for p in ([paths] if isinstance(paths, (str, bytes, os.PathLike)) else paths)]
    arr = (C.c_char_p * len(paths))(*paths)
    return _run(lambda lib, *a: lib.smg_count_files_parts(arr, len(paths), *a), k, t, device, threads, partitions, max_entries, gzip, dump)


def count_bases(seq, k, t=4, device=0, threads=4, partitions=0, max_entries=0):
    """The same from sequence bytes (bytes or a uint8 array) in which any byte outside ACGTacgt separates."""
    buf = np.ascontiguousarray(np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray, memoryview)) else seq,
                               dtype=np.uint8)
    return _run(lambda lib, *a: lib.smg_count_bases_parts(buf.ctypes.data_as(C.c_void_p), buf.size, *a), k, t, device, threads,
                partitions, max_entries)


class DeviceTable:
    """A counted table that stayed in device memory: k, t, nels, words (64-bit words per k-mer) and the two device pointers
    keys_ptr (uint64[nels * words], left aligned, sorted) and counts_ptr (uint16[nels]), in the layout of engine.Engine.bind.
    close() -- or leaving the `with` block -- frees them."""

    def __init__(self, k, t, nels, words, keys_ptr, counts_ptr, device=0):
        self.k, self.t, self.nels, self.words, self.device = int(k), int(t), int(nels), int(words), int(device)
        self.keys_ptr, self.counts_ptr = keys_ptr, counts_ptr

    def close(self):
        for name in ("keys_ptr", "counts_ptr"):
            if getattr(self, name, None) and _lib is not None:
                _lib.smg_count_device_free(getattr(self, name))
            setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close

    def to_host(self):
        """(k-mers uint64[nels, words], counts uint16[nels]) copied from the device"""
        from . import engine
        e = engine.Engine(self.device)
        try:
            e.bind(self.k, self.nels, self.keys_ptr, self.counts_ptr)
            return e.table_host()
        finally:
            e.close()


def _run_device(call, k, t, device, threads, partitions, max_entries, gzip=False, dump=False):
    lib = load_library()
    opts = DumpOpts(int(k), int(t), int(device), int(threads), 0, int(bool(gzip)), int(bool(dump)))
    parts = Parts(int(partitions), int(max_entries), 0, 0, 0.0, 0.0)
    keys, cnt = C.c_void_p(), C.c_void_p()
    nels, words = C.c_int64(0), C.c_int(0)
    hist = np.zeros(HIST, dtype=np.uint64)
    st = Stats()
    err = C.create_string_buffer(1024)
    rc = call(lib, C.byref(opts), C.byref(parts), C.byref(keys), C.byref(cnt), C.byref(nels), C.byref(words),
              hist.ctypes.data_as(C.c_void_p), C.byref(st), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    stats = st.asdict()
    stats.update(used=parts.used, store_bytes=parts.store_bytes, ms_pack=parts.ms_pack, ms_plan=parts.ms_plan, split=parts.split)
    return DeviceTable(k, t, nels.value, words.value, keys.value, cnt.value, device), hist, stats


def _as_bases(seq):
    return np.ascontiguousarray(np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray, memoryview)) else seq,
                                dtype=np.uint8)


def count_files_device(paths, k, t=4, device=0, threads=4, partitions=0, max_entries=0, gzip=False, dump=False):
    """count_files with the table left on the device -> (DeviceTable, hist uint64[32768], stats dict)"""
    paths = [os.fsencode(p) for p in ([paths] if isinstance(paths, (str, bytes, os.PathLike)) else paths)]
    arr = (C.c_char_p * len(paths))(*paths)
    return _run_device(lambda lib, *a: lib.smg_count_files_device(arr, len(paths), *a), k, t, device, threads, partitions, max_entries,
                       gzip, dump)


def count_bases_device(seq, k, t=4, device=0, threads=4, partitions=0, max_entries=0):
    """count_bases with the table left on the device -> (DeviceTable, hist uint64[32768], stats dict)"""
    buf = _as_bases(seq)
    return _run_device(lambda lib, *a: lib.smg_count_bases_device(buf.ctypes.data_as(C.c_void_p), buf.size, *a), k, t, device, threads,
                       partitions, max_entries)


def reads_to_plot(paths_or_bases, k, t, e, device=0, threads=4, partitions=0, max_entries=0, symcheck="hash", gzip=False, dump=False):
    """Reads to the het-mer plot in one process: count on the device (k-mers with count >= t), hand the table over where
    it lies, trim at e, close under reverse complement, run -> (plot int64[1001, 501], hist uint64[32768], stats dict).
    The closed table runs in core, or, where it is beyond one engine or the memory, in prefix shards one after the other
    (engine.run_device_mode says which).
    paths_or_bases: sequence bytes (bytes, bytearray, memoryview or a uint8 array) or one path or a list of paths.
    gzip: read plain gzip files too, as count_files does.  dump: the files are k-mer dumps, as count_files reads them.
    e < t cannot be honoured (the entries below t are gone) and raises ValueError.  The stats are the counter's, with the
    engine's under "hetmers"."""
    from . import engine
    if int(e) < int(t):
        raise ValueError(f"e = {e} is below t = {t}: the k-mers with a count below t are not in the table")
    if isinstance(paths_or_bases, (bytes, bytearray, memoryview, np.ndarray)):
        if dump:
            raise ValueError("dump=True reads files: a buffer of sequence bytes is no k-mer dump")
        got = count_bases_device(paths_or_bases, k, t, device, threads, partitions, max_entries)
    else:
        got = count_files_device(paths_or_bases, k, t, device, threads, partitions, max_entries, gzip, dump)
    table, hist, stats = got
    with table:
        plot, est = engine.hetmers_run_device(k, table.nels, table.keys_ptr, table.counts_ptr, device=device, symcheck=symcheck,
                                              condition=engine.COND_TRIM | engine.COND_SYMM, ethresh=int(e))
    stats["hetmers"] = est
    return plot, hist, stats


def plan(windows, budget, partitions=0):
    """Host only: the cuts of a partitioned run over the 4096-bin window histogram -> int32 array, range r is bins
    cuts[r] .. cuts[r + 1] - 1.  Raises CountError (-3) with the bin named when one bin alone is above the budget."""
    lib = load_library()
    w = np.ascontiguousarray(windows, dtype=np.uint64)
    if w.shape != (BINS,):
        raise ValueError(f"windows must have {BINS} entries")
    cuts = np.zeros(BINS + 1, dtype=np.int32)
    n = C.c_int32(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_plan(w.ctypes.data_as(C.c_void_p), int(budget), int(partitions), cuts.ctypes.data_as(C.c_void_p), C.byref(n),
                            err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    return cuts[: n.value + 1].copy()


def plan_fine(windows, split, sub, budget):
    """Host only: the cuts where `plan` refuses a single bin.  split: the bins that are split, ascending; sub[s] = the 4096
    windows of bin split[s] by its next 12 bits.  -> int32 array of values of the leading 24 bits, range r is
    cuts[r] .. cuts[r + 1] - 1, cuts[-1] = 2^24; a cut that is no multiple of 4096 lies inside a split bin.  Raises
    CountError (-3) with bin and sub-bin named when one sub-bin alone is above the budget."""
    lib = load_library()
    w = np.ascontiguousarray(windows, dtype=np.uint64)
    if w.shape != (BINS,):
        raise ValueError(f"windows must have {BINS} entries")
    b = np.ascontiguousarray(split, dtype=np.int32).reshape(-1)
    s = np.ascontiguousarray(sub, dtype=np.uint64)
    if s.shape != (len(b), BINS):
        raise ValueError(f"sub must have {BINS} entries for each of the {len(b)} split bins")
    room = min(2 * (int(w.astype(object).sum()) // max(int(budget), 1)) + 5, FINE_BINS + 1)
    cuts = np.zeros(room, dtype=np.int32)
    n = C.c_int32(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_plan_fine(w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), len(b), s.ctypes.data_as(C.c_void_p),
                                 int(budget), cuts.ctypes.data_as(C.c_void_p), room, C.byref(n), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    return cuts[: n.value + 1].copy()


def memory_plan(k, free_bytes, bound, partitions=0, max_entries=0, batch_bases=0):
    """Host only: how a run would share out `free_bytes` of device memory for an input of at most `bound` sequence bytes
    (smg_count_memory_plan; no device, no environment: the function the counting calls use) -> dict with `cap` (positions of
    a batch), `parted` (bool: packed and counted by key range) and `store_cap` (positions of the store, 0 for one pass).
    batch_bases is the value of the test hook SMG_COUNT_BATCH_BASES, 0 for none.  Raises CountError (-3) where it does not fit."""
    lib = load_library()
    cap, parted, store = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_memory_plan(int(k), int(free_bytes), int(bound), int(partitions), int(max_entries), int(batch_bases),
                                   C.byref(cap), C.byref(parted), C.byref(store), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    return {"cap": cap.value, "parted": bool(parted.value), "store_cap": store.value}


def stream_plan(k, free_bytes, known_bound=0, partitions=0, max_entries=0, batch_bases=0, store_bases=0):
    """Host only: the plan of a call that reads at least one stream and so has no bound (smg_count_stream_plan; no device, no
    environment: the function such a call uses) -> dict as memory_plan's.  known_bound covers the regular files of the call.
    partitions == 1 is one pass (`parted` False, `store_cap` 0) with a batch that is never clamped to the input; any other
    value packs the batches into a store that BEGINS with `store_cap` positions -- store_bases (the test hook
    SMG_COUNT_STREAM_STORE) rounded up to whole tiles of 4096, by default 2^30 or what memory_plan gives known_bound where that
    is more -- and grows by half from there.  With no stream in the call it is memory_plan that decides, as it always did.
    Raises CountError (-2) for bad arguments, (-3) where the first store or the batch does not fit."""
    lib = load_library()
    cap, parted, store = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_stream_plan(int(k), int(free_bytes), int(known_bound), int(partitions), int(max_entries), int(batch_bases),
                                   int(store_bases), C.byref(cap), C.byref(parted), C.byref(store), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    return {"cap": cap.value, "parted": bool(parted.value), "store_cap": store.value}


def parse(path) -> bytes:
    """Host only: the stripped byte stream of one plain FASTA / FASTQ file or stream ("-", a FIFO, /dev/stdin), one '\\n'
    between two records.  BGZF is refused here (CountError -2): there is no device in this call, see bgzf_inflate."""
    lib = load_library()
    seq, n = C.c_void_p(), C.c_int64(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_parse(os.fsencode(path), C.byref(seq), C.byref(n), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        return C.string_at(seq, n.value)
    finally:
        lib.smg_count_free(seq)


def bgzf_scan(path) -> dict:
    """Host only: the members of a BGZF file, walked from header to header -> {"blocks": members (empty ones and the EOF
    marker included), "text_bytes": the sum of their ISIZE fields}.  Raises CountError: -2 for a file that is not BGZF, -4
    with the offset of the block for a file that is cut off or whose headers do not fit it."""
    lib = load_library()
    blocks, text = C.c_int64(0), C.c_int64(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_bgzf_scan(os.fsencode(path), C.byref(blocks), C.byref(text), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    return {"blocks": blocks.value, "text_bytes": text.value}


def bgzf_inflate(path, device=0):
    """The text of a whole BGZF file, inflated on the device as the counting calls inflate it -> (bytes, ms_kernel: the sum
    of the HIP-event times of the launches).  Raises CountError -4 with the offset of the first member that does not
    inflate to its ISIZE bytes with the CRC-32 of its trailer, and the reason."""
    lib = load_library()
    text, n, ms = C.c_void_p(), C.c_int64(0), C.c_double(0.0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_bgzf_inflate(os.fsencode(path), int(device), C.byref(text), C.byref(n), C.byref(ms), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        return C.string_at(text, n.value), ms.value
    finally:
        lib.smg_count_free(text)


def gzip_inflate(path, span_bytes=0, device=0):
    """The text of a whole gzip file by the route of the counting calls with gzip=True: the index of its restart points on the
    device, then the exact decoder over it -> (bytes, (ms finder + marker decoder, ms resolver, ms exact decoder): HIP events).
    span_bytes: compressed bytes of a span, 1024 .. 1048576, 0 for the default.  Raises CountError -2 for a file that is not
    gzip, -4 "<path>: gzip member at offset <o>: ..." or "<path>: deflate block at offset <o>: ..." for one that is damaged."""
    lib = load_library()
    text, n, ms = C.c_void_p(), C.c_int64(0), (C.c_double * 3)()
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_gzip_inflate(os.fsencode(path), int(device), int(span_bytes), C.byref(text), C.byref(n), ms, err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        return C.string_at(text, n.value), tuple(ms)
    finally:
        lib.smg_count_free(text)


def gzip_text_host(path, span_bytes=0) -> bytes:
    """Host only: the same text by the same block finder, marker decoder, chain, resolver and exact decoder, run as one lane
    on the host.  A test twin, not a fallback of the counting calls.  Errors as gzip_inflate."""
    lib = load_library()
    text, n = C.c_void_p(), C.c_int64(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_gzip_text_host(os.fsencode(path), int(span_bytes), C.byref(text), C.byref(n), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        return C.string_at(text, n.value)
    finally:
        lib.smg_count_free(text)


def gzip_report(path) -> dict:
    """Host only: what the last call of this process that reads plain gzip (count_files* with gzip=True, gzip_inflate,
    gzip_text_host) read of the file it was given as `path` -> {"members", "text_bytes", "spans", "linked", "repaired",
    "ms_marker", "ms_resolve", "ms_exact"}.  Raises CountError -2 where it read no such file."""
    lib = load_library()
    v = [C.c_int64(0) for _ in range(5)]
    ms = (C.c_double * 3)()
    rc = lib.smg_count_gzip_report(os.fsencode(path), *[C.byref(x) for x in v], ms)
    if rc != 0:
        raise CountError(rc, f"the last call read no gzip file {path}")
    return {"members": v[0].value, "text_bytes": v[1].value, "spans": v[2].value, "linked": v[3].value, "repaired": v[4].value,
            "ms_marker": ms[0], "ms_resolve": ms[1], "ms_exact": ms[2]}


def _dump_call(call, n_ms=0):
    lib = load_library()
    keys, cnt, n, words = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int(0)
    ms = C.c_double(0.0)
    err = C.create_string_buffer(1024)
    rc = call(lib, C.byref(keys), C.byref(cnt), C.byref(n), C.byref(words), *([C.byref(ms)] if n_ms else []), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        m, w = n.value, words.value
        k64 = np.ctypeslib.as_array(C.cast(keys, C.POINTER(C.c_uint64)), shape=(max(m, 1) * w,))[: m * w].copy().reshape(m, w)
        c32 = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint32)), shape=(max(m, 1),))[:m].copy()
    finally:
        lib.smg_count_free(keys)
        lib.smg_count_free(cnt)
    return k64, c32, ms.value


def dump_parse(path, k):
    """Host only, plain files and plain streams only: the records of a k-mer dump by the line decoder the kernel compiles, run on the host ->
    (k-mers uint64[n, words], canonical, left aligned; counts uint32[n], saturated at 2^32 - 1), in line order.  A test twin,
    not a fallback.  Raises CountError -2 for a text that does not begin with a base, -4 "<path>: dump line at offset <o>:
    <reason>" for the first bad line."""
    k64, c32, _ = _dump_call(lambda lib, *a: lib.smg_count_dump_parse(os.fsencode(path), int(k), *a))
    return k64, c32


def dump_records(path, k, device=0, gzip=False):
    """The same records as the kernel of the counting calls emits them, by the route those calls take (plain, BGZF, with
    gzip=True plain gzip), in no particular order -> (k-mers, counts, ms_kernel: the HIP-event time of the line kernel).
    Errors as dump_parse."""
    return _dump_call(lambda lib, *a: lib.smg_count_dump_records(os.fsencode(path), int(k), int(device), int(bool(gzip)), *a), n_ms=1)


def bam_text(text, piece=0) -> bytes:
    """Host only: the stripped stream of inflated BAM text (the primary records' bases through "=ACMGRSVTWYHKDBN", one '\\n'
    between two of them), fed to the framer of the counting calls in pieces of `piece` bytes (0: one piece) and unpacked by
    the host routine.  Raises CountError -4, "<text>: BAM header: ..." or "<text>: BAM record at text offset <o>: ...", for a
    negative length field, a block_size too small for its fields and a text that ends inside the header or a record."""
    lib = load_library()
    buf = bytes(text)
    seq, n = C.c_void_p(), C.c_int64(0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_bam_text(C.cast(C.c_char_p(buf), C.c_void_p), len(buf), int(piece), C.byref(seq), C.byref(n), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        return C.string_at(seq, n.value)
    finally:
        lib.smg_count_free(seq)


def bam_strip(path, device=0):
    """The stripped stream of a whole BAM file by the route of the counting calls: inflated on the device, framed on the
    host, unpacked on the device -> (bytes, contributing records, ms_kernel: the HIP-event time of the unpack kernel alone).
    Raises CountError -2 for a file that is not BAM, -4 as bgzf_inflate and bam_text do."""
    lib = load_library()
    seq, n, rec, ms = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_double(0.0)
    err = C.create_string_buffer(1024)
    rc = lib.smg_count_bam_strip(os.fsencode(path), int(device), C.byref(seq), C.byref(n), C.byref(rec), C.byref(ms), err, len(err))
    if rc != 0:
        raise CountError(rc, err.value.decode(errors="replace"))
    try:
        return C.string_at(seq, n.value), rec.value, ms.value
    finally:
        lib.smg_count_free(seq)


def bam_report(path) -> dict:
    """Host only: what the last call of this process that reads BAM (count_files*, bam_strip) read from the BAM file it was
    given as `path` -> {"records", "bases", "ms_frame" (host clock), "ms_inflate", "ms_unpack" (HIP events of the two kernels),
    "ms_d2h" (host clock: the stripped bytes to the host)}.  Raises CountError -2 where it read no such file to its end."""
    lib = load_library()
    rec, bases, ms = C.c_int64(0), C.c_int64(0), (C.c_double * 4)()
    rc = lib.smg_count_bam_report(os.fsencode(path), C.byref(rec), C.byref(bases), ms)
    if rc != 0:
        raise CountError(rc, f"the last call read no BAM file {path} to its end")
    return {"records": rec.value, "bases": bases.value, "ms_frame": ms[0], "ms_inflate": ms[1], "ms_unpack": ms[2], "ms_d2h": ms[3]}
