"""An N = 3 tiny-capacity case for the replica-per-rank runs of
test_replica_gloo.py, added to its CASES when this module is imported.

N = 3 is the group size whose fast steps run in the summary-word form on the
device (k_fast_both, rbe_fast.h lead_gather_slot / foll_gather_slot); the
host build steps that form with SoaCpu(staged=4), which the HIP engine has no
argument for, so the case's engine arguments depend on the tier.  The ranks
are spawned processes that import the module of their entry point: aux_worker
below, so that the case exists there too."""
import test_replica_gloo as RG

# C4-shaped, every replica of a group on its own rank, every capacity minimal
C4_TINY = dict(n_groups=30, n_replicas=3, quiesce=True, wl_enabled=True, wl_start_round=30,
               wl_active_mod=2, wl_read_permille=900)
TINY = dict(maxm=1, ecap=1, rtr_cap=1, dri_cap=1, rq_cap=1, ring=8)
NAME = "C4_tiny_w3"


def register(gpu):
    RG.CASES[NAME] = (C4_TINY, 3, 300, dict(TINY) if gpu else dict(TINY, staged=4))


register(False)


def aux_worker(rank, world, port, name, gpu, trace, q, fixed=False):
    register(gpu)
    RG._worker(rank, world, port, name, gpu, trace, q, fixed)


def run_aux_case(monkeypatch, gpu=False, trace=True):
    """test_replica_gloo.run_case of the case, its ranks entering through aux_worker."""
    monkeypatch.setattr(RG, "_worker", aux_worker)
    RG.run_case(NAME, gpu=gpu, trace=trace)
