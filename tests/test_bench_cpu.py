"""bench.py --dump-outputs without a device: what it writes of a state, in what form, within what size."""
import importlib.util
import os

import numpy as np

import common as cm


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(cm.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class _Ctx:
    """Stands in for a device context: download fills the state the way mckpp_hip_download would."""

    def __init__(self):
        self.masks = []

    def download(self, k3, mask):
        self.masks.append(mask)
        for f in ("U", "X", "hmix", "kmix", "difs"):
            a = getattr(k3, f)
            a[...] = np.arange(a.size, dtype=np.float64).reshape(a.shape, order="F")

    def synchronize(self):
        pass


def test_dump_outputs_writes_the_state_float64_on_a_fixed_sample(tmp_path):
    import mckpp_f90_amd as mk

    bench = _bench()
    ncol, nz = 5000, 100
    kc, k3 = cm.make_hip_case(ncol, nz)
    npass = (np.arange(ncol, dtype=np.int32) % 7) + 6
    dirs = []
    for run in range(2):
        ctx = _Ctx()
        d = str(tmp_path / f"run{run}")
        bench.dump_outputs(d, mk, ctx, k3, npass)
        assert ctx.masks == [mk.api.F_ALL]
        dirs.append(d)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"hmix.npy", "kmix.npy", "npasses.npy", "sample_columns.npy"} <= set(names)
    assert {f"sample_{f}.npy" for f in bench.DUMP_FIELDS} <= set(names)
    assert sum(os.path.getsize(os.path.join(dirs[0], n)) for n in names) <= bench.DUMP_BYTES
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype == np.float64 and np.array_equal(a, b), n
    cols = np.load(os.path.join(dirs[0], "sample_columns.npy")).astype(np.int64)
    assert len(cols) == 2048 and np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < ncol
    assert np.array_equal(np.load(os.path.join(dirs[0], "sample_X.npy")), k3.X[cols])
    assert np.array_equal(np.load(os.path.join(dirs[0], "hmix.npy")), k3.hmix)
    assert np.array_equal(np.load(os.path.join(dirs[0], "npasses.npy")), npass)
