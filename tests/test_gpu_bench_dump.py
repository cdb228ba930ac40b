"""bench.py --dump-outputs: what dump_outputs writes for the bench's C4 path
(settle, prepare_run, run_timed) is float64, within the 64 MB bound, agrees
with the engine's own per-replica calls, and is identical for two engines
built from the same arguments (what makes two builds comparable)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("replicas", "updates", "views", "messages", "ready_to_reads", "counters")
GROUPS = 3000  # 5 whole sample blocks of 512 groups and one of 440


def _run(out_dir):
    import bench
    from dragonboat_amd.engine import Engine, make_config
    kw, settle, _ = bench.WORKLOADS["c4"]
    eng = Engine(make_config(device=0, trace=False, **dict(kw, n_groups=GROUPS)))
    eng.run(settle + 3)
    eng.prepare_run(5)
    eng.sync()
    eng.reset_counters()
    eng.run_timed(5)
    c = eng.counters()
    bench.dump_outputs(eng, str(out_dir), c)
    return eng, c


def test_gpu_bench_dump_outputs(gpu_available, tmp_path):
    from dragonboat_amd.engine import COUNTER_NAMES
    eng, c = _run(tmp_path / "a")
    eng2, _ = _run(tmp_path / "b")
    eng2.close()
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in NAMES}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in NAMES}
    cols = json.load(open(tmp_path / "a" / "columns.json"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted([f"{n}.npy" for n in NAMES] +
                                                       ["columns.json"])
    assert sum(x.nbytes for x in a.values()) <= 64_000_000
    for n in NAMES:
        assert a[n].dtype == np.float64 and a[n].ndim == 2
        assert a[n].shape[1] == len(cols[n])
        assert np.array_equal(a[n], b[n]), n  # same arguments, same arrays
    # every replica of every group: 3000 groups fit in the sample's 32 blocks
    rep = a["replicas"][:, 0].astype(np.int64)
    assert np.array_equal(rep, np.arange(eng.n_rep))
    assert len(a["updates"]) == len(a["views"]) == eng.n_rep
    # against the engine's per-replica calls, for replicas across the blocks
    ucol, vcol, mcol = (cols[k] for k in ("updates", "views", "messages"))
    ups, views = eng.updates(), eng.views()
    for r in (0, 1, 30, 1535, 1536, 4607, 7680, eng.n_rep - 1):
        for f in ("term", "commit", "n_messages", "n_ready_to_read", "flags", "leader_id"):
            assert a["updates"][r, ucol.index(f)] == getattr(ups[r], f), (r, f)
        for f in ("term", "committed", "last_index", "role"):
            assert a["views"][r, vcol.index(f)] == getattr(views[r], f), (r, f)
        assert a["views"][r, vcol.index("match[2]")] == views[r].match[2]
        got = a["messages"][a["messages"][:, 0] == r]
        ref = eng.messages(r)
        assert len(got) == len(ref)
        for g, m in zip(got, ref):
            assert (g[mcol.index("type")], g[mcol.index("to")], g[mcol.index("log_index")]) == \
                (m.type, m.to, m.log_index)
        rtr = a["ready_to_reads"][a["ready_to_reads"][:, 0] == r][:, 1:]
        assert [tuple(x) for x in rtr.tolist()] == [tuple(map(float, x))
                                                    for x in eng.ready_to_reads(r)]
    assert len(a["messages"]) > 0 and len(a["ready_to_reads"]) > 0  # C4 reads and proposes
    assert a["counters"][0].tolist() == [float(c[k]) for k in COUNTER_NAMES]
    eng.close()
