"""Output files that appear whole or not at all.  No dependency beyond the standard library."""
import os
import threading


def write_atomic(path, content, mode="w"):
    """Write through a temporary file in the same directory and rename it into place: concurrent replicate workers (and a
    reader of a half-finished run) never see a truncated file.  `content` is the text or bytes, or a function of the open file."""
    tmp = f"{path}.tmp{os.getpid()}_{threading.get_ident()}"     # replicate fits may share a process (one thread each)
    with open(tmp, mode) as fh:
        content(fh) if callable(content) else fh.write(content)
    os.replace(tmp, path)
