"""Helper of the stream tests: a FIFO (os.mkfifo) with a writer thread that writes in pieces, joined with a time limit so
that a reader that fails cannot hang a test.  A helper module, not a test."""
import os
import threading

import pytest

from smudgeplot_amd import count


class Writer(threading.Thread):
    """writes `data` into the FIFO at `path` in pieces of `piece` bytes; .error is what ended it early, .wrote the bytes it
    got rid of.  finish() joins it, with a time limit, and lets go of a writer whose reader never came."""

    def __init__(self, path, data, piece):
        super().__init__(daemon=True)
        self.path, self.data, self.piece = str(path), data, piece
        self.error, self.wrote = None, 0
        self.start()

    def run(self):
        try:
            fd = os.open(self.path, os.O_WRONLY)
            try:
                view = memoryview(self.data)
                for at in range(0, len(view), self.piece):
                    chunk = view[at:at + self.piece]
                    while len(chunk):
                        n = os.write(fd, chunk)
                        self.wrote += n
                        chunk = chunk[n:]
            finally:
                os.close(fd)
        except OSError as e:                                     # (BrokenPipeError: the reader went away)
            self.error = e

    def finish(self, wait=20):
        """wait: seconds given to a writer whose reader is still at work (0 where the reader is known never to have come)"""
        self.join(wait)
        if self.is_alive():                                      # nobody opened the FIFO: open it, so that the writer's open returns,
            fd = os.open(self.path, os.O_RDONLY | os.O_NONBLOCK)
            self.join(2)                                          # and close it, so that a write that waits for room fails
            os.close(fd)
            self.join(10)
        assert not self.is_alive(), "the writer hangs"
        return self


def fifo(tmp_path, name):
    path = tmp_path / name
    if not path.exists():
        os.mkfifo(path)
    return path


def through_fifo(tmp_path, data, piece, call, name="in.fifo"):
    """call(path of a FIFO into which `data` is written) -> its result; the writer wrote everything and saw no error"""
    path = fifo(tmp_path, name)
    w = Writer(path, data, piece)
    try:
        got = call(str(path))
    finally:
        w.finish()
    assert w.error is None and w.wrote == len(data), (w.error, w.wrote)
    return got


def refused(tmp_path, data, call, name="bad.fifo"):
    """call(FIFO) raises CountError -> the exception; the writer is let go of whatever became of it"""
    path = fifo(tmp_path, name)
    w = Writer(path, data, 4096)
    try:
        with pytest.raises(count.CountError) as e:
            call(str(path))
    finally:
        w.finish()
    return e.value
