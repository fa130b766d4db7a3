"""What the GPU tests share for reading the library's ILUPP_DEBUG lines: an environment variable set for a block, and what the library
writes to file descriptor 2 during a block (the library prints from C, past sys.stderr; child processes have no capfd)."""
import os
import sys
import tempfile


class Stderr:
    """what the library writes to file descriptor 2 during the block (the child processes have no capfd)"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.err = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()


class Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
