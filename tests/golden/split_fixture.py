"""Keep every fixture file under the size limit of a committed file (1 MiB).

`split_fixture(path)` rewrites an .npz that is larger as `<name>.npz` plus `<name>.part<k>.npz`, each under the
limit, the arrays unchanged; tests/conftest.py::golden(name) merges the parts again.  The generators call it on what
they write:

    python tests/golden/split_fixture.py tests/golden/<name>.npz
"""
import glob
import io
import os
import sys

import numpy as np

LIMIT = 1 << 20
BUDGET = 900_000            # bytes per part: room for the archive's own overhead under LIMIT


def _compressed_size(key, a):
    buf = io.BytesIO()
    np.savez_compressed(buf, **{key: a})
    return buf.tell()


def split_fixture(path):
    """Returns the files that now hold the fixture."""
    stem = path[:-len(".npz")]
    for old in glob.glob(glob.escape(stem) + ".part*.npz"):
        os.remove(old)
    if os.path.getsize(path) <= LIMIT:
        return [path]
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    parts, sizes = [], []
    for k in arrays:                                     # first fit, in the archive's own key order
        s = _compressed_size(k, arrays[k])
        if s > BUDGET:
            raise ValueError(f"{path}: array {k!r} alone takes {s} bytes compressed")
        for i, used in enumerate(sizes):
            if used + s <= BUDGET:
                parts[i].append(k)
                sizes[i] += s
                break
        else:
            parts.append([k])
            sizes.append(s)
    files = [path] + [f"{stem}.part{i}.npz" for i in range(1, len(parts))]
    for f, keys in zip(files, parts):
        np.savez_compressed(f, **{k: arrays[k] for k in keys})
        assert os.path.getsize(f) <= LIMIT, f
    return files


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print(p, "->", [f"{os.path.basename(f)} {os.path.getsize(f)}" for f in split_fixture(p)])
