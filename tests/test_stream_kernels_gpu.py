"""The pass bookkeeping kernels on their own, against the host models of stream_model.py:
conv.hip conv_update_kernel (stop rule, device pass counting, gate, host-mapped flag slots),
stream.hip stream_plan_kernel / stream_copy_kernel (ops.stream_swap) and
stream_publish_kernel (ops.stream_publish with ops.HostMailbox).

Every test builds its tensors by hand and calls the ops wrapper directly; no solver runs.
Integer state is compared exactly and every tensor of a swap bit for bit, padding
included.  The errors of conv_update may differ from the model by the device sqrt alone
(the radicand is the same float64 on both sides): the cap is 2 ulp.

Largest distance observed on an MI355X over all cases of this file: 0 ulp."""
import functools
import itertools

import numpy as np
import pytest
import torch

from cnmf_torch_amd import ops
from cnmf_torch_amd.ops import reference

import stream_model as sm

pytestmark = pytest.mark.gpu

ULP_CAP = 2
_seen = {"ulp": 0}


def _ulp(dev, model, what):
    d = sm.ulp_distance(dev, model)
    _seen["ulp"] = max(_seen["ulp"], d)
    assert d <= ULP_CAP, (what, d)
    return d


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


# ------------------------------------------------------------------------------ conv_update
@functools.lru_cache(maxsize=None)
def _conv_inputs(n):
    x_sq, lins, quads, exact = sm.conv_inputs(n)
    return x_sq, lins, quads, exact, [_cuda(a) for a in lins], [_cuda(a) for a in quads]


def _conv_compare(st_d, st_m, what):
    for k in ("active", "converged", "n_pass"):
        got = st_d[k].cpu().numpy()
        assert got.dtype == st_m[k].dtype and np.array_equal(got, st_m[k]), (what, k, got, st_m[k])
    for k in ("err_init", "err_prev", "err"):
        _ulp(st_d[k].cpu().numpy(), st_m[k], (what, k))


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("tol", [0.0, 1e-4])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 700])
def test_conv_update_matches_model(n, tol, mode):
    x_sq, lins, quads, exact, lins_d, quads_d = _conv_inputs(n)
    for use_gate, use_flags in itertools.product([False, True], repeat=2):
        st_m = sm.conv_state(n)
        st_r = {k: torch.from_numpy(v.copy()) for k, v in st_m.items()}
        st_d = {k: _cuda(v) for k, v in st_m.items()}
        gate_m, gate_d = np.array([5], np.int32), _cuda(np.array([5], np.int32))
        flags_m, ctr_m = np.full((2, n), -1, np.int32), np.zeros(1, np.int32)
        flags_d = torch.full((2, n), -1, dtype=torch.int32).pin_memory()
        ctr_d = torch.zeros(1, dtype=torch.int32, device=lins_d[0].device)
        for p, (pass_idx, final, init, max_pass) in enumerate(sm.conv_protocol(mode)):
            what = (n, tol, mode, use_gate, use_flags, p)
            before = {k: v.copy() for k, v in st_m.items()}
            slot = int(ctr_m[0]) & 1
            other = flags_d[1 - slot].clone()
            rel = sm.conv_update_model(lins[p], quads[p], x_sq, st_m, n, pass_idx, tol, final,
                                       init=init, max_pass=max_pass,
                                       gate=gate_m if use_gate else None,
                                       host_flags=(flags_m, ctr_m) if use_flags else None)
            if not init:
                sm.check_margin(rel, tol, exact[p])
            reference.conv_update(torch.from_numpy(lins[p]), torch.from_numpy(quads[p]), x_sq,
                                  st_r, n, pass_idx, tol, final, init=init, max_pass=max_pass)
            ops.conv_update(lins_d[p], quads_d[p], x_sq, st_d, n, pass_idx, tol, final, init=init,
                            gate=gate_d if use_gate else None, max_pass=max_pass,
                            host_flags=(flags_d, ctr_d) if use_flags else None)
            torch.cuda.synchronize()
            _conv_compare(st_d, st_m, what)
            for k in st_m:          # the float64 reference and the model: bitwise
                assert st_r[k].numpy().tobytes() == st_m[k].tobytes(), (what, k)
            assert gate_d.item() == gate_m[0], what
            assert ctr_d.item() == ctr_m[0], what
            assert np.array_equal(flags_d.numpy(), flags_m), what
            assert torch.equal(flags_d[1 - slot], other), what     # the slot not written
            if use_flags:
                assert np.array_equal(flags_m[slot], st_m["active"]) and ctr_m[0] == p + 1
            if not init and not before["active"].any():
                # nothing was active: the state is untouched, the gate drops
                for k in st_m:
                    assert st_d[k].cpu().numpy().tobytes() == before[k].tobytes(), (what, k)
                assert gate_m[0] == (0 if use_gate else 5)
        assert not st_m["active"].any()
        if mode == "device":
            assert st_m["n_pass"].max() == 3 and p == sm.CONV_PASSES
    print(f"conv_update n={n} tol={tol} {mode}: largest ulp distance so far {_seen['ulp']}")


def test_conv_update_all_inactive_touches_nothing():
    n = 300
    rng = np.random.default_rng(3)
    st_m = {"err_init": rng.random(n) + 1, "err_prev": rng.random(n), "err": rng.random(n),
            "active": np.zeros(n, np.int32), "converged": rng.integers(0, 2, n).astype(np.int32),
            "n_pass": rng.integers(1, 9, n).astype(np.int32)}
    st_d = {k: _cuda(v) for k, v in st_m.items()}
    lin = torch.rand(n, device="cuda")
    quad = torch.rand(n, device="cuda")
    gate = _cuda(np.array([1], np.int32))
    flags = torch.full((2, n), -1, dtype=torch.int32).pin_memory()
    ctr = _cuda(np.array([3], np.int32))
    ops.conv_update(lin, quad, 50.0, st_d, n, -1, 1e-4, False, gate=gate, max_pass=4,
                    host_flags=(flags, ctr))
    torch.cuda.synchronize()
    for k in st_m:
        assert st_d[k].cpu().numpy().tobytes() == st_m[k].tobytes(), k
    assert gate.item() == 0 and ctr.item() == 4
    assert flags.tolist() == [[-1] * n, [0] * n]


# ------------------------------------------------------------------------------ stream_swap
def _to_device(w):
    return {k: (v if k == "geo" else _cuda(v)) for k, v in w.items()}


def _to_host(d):
    return {k: (v if k == "geo" else v.cpu().numpy()) for k, v in d.items()}


def _swap_both(w, chunks, what):
    """One ops.stream_swap on a device copy of the numpy world, the model on the world
    itself, and every base buffer compared bit for bit.  Returns the world before."""
    before = {k: (v if k == "geo" else v.copy()) for k, v in w.items()}
    d = _to_device(w)
    ops.stream_swap(*sm.swap_views(d), chunks=chunks)
    torch.cuda.synchronize()
    sm.stream_swap_model(*sm.swap_views(w))
    sm.assert_worlds_equal(_to_host(d), w, what)
    return before


def _copy_world(**kw):
    """Six positions: 1, 2, 4, 5 stopped, three replicates staged -- 1, 2, 4 are harvested
    and refilled, 5 is harvested and left empty, 0 and 3 are not touched."""
    geo = dict(n=6, qc=4, R=9)
    geo.update(kw)
    w = sm.make_world(**geo)
    sm.stage(w, [6, 7, 8])
    sm.set_stopped(w, [1, 2, 4, 5])
    return w


COPY_CASES = {
    "vector": dict(K=7, G=64, N=128, Gp=64),
    "scalar_by_columns": dict(K=7, G=61, N=33, Gp=40),
    "vector_pitch_68": dict(K=7, G=64, N=32, ldw=68, ldh=36, Gp=37),
    "scalar_by_pitch_65": dict(K=7, G=64, N=32, ldw=65, ldh=33, Gp=64, pl_ld=72),
    "scalar_by_batch_base": dict(K=7, G=64, N=32, w_off=1, Gp=40, pl_ld=48),
    "scalar_by_store_base": dict(K=7, G=64, N=32, ow_off=1, Gp=37, pl_ld=41),
    "empty_slices_scalar": dict(K=1, G=3, N=0, store_ht=False, Gp=37),
    "empty_slices_vector": dict(K=1, G=8, N=4, Gp=40, S=2),
    "store_without_usages": dict(K=3, G=12, N=20, store_ht=False, Gp=64, S=2),
}


@pytest.mark.parametrize("chunks", [1, 32])
@pytest.mark.parametrize("case", sorted(COPY_CASES))
def test_stream_swap_copy_paths(case, chunks):
    w = _copy_world(**COPY_CASES[case])
    g = w["geo"]
    # the premises of the case: what decides between 16-byte vectors and scalars
    ptr = sm.swap_views(_to_device(w))
    aligned = [t.data_ptr() % 16 == 0 for t in (ptr[0]["W"], ptr[1]["W"], ptr[2]["W"])]
    vec = g["G"] % 4 == 0 and g["ldw"] % 4 == 0 and all(aligned)
    assert vec == case.startswith(("vector", "empty_slices_vector", "store_without")), aligned
    if case == "scalar_by_batch_base":
        assert aligned == [False, True, True]
    if case == "scalar_by_store_base":
        assert aligned == [True, True, False]
    before = _swap_both(w, chunks, (case, chunks))
    assert w["occ"].tolist() == [0, 6, 7, 3, 8, -1] and w["done"][0] == 4 and w["gate"][0] == 1
    assert w["plan"].tolist() == [-1, 0, 1, -1, 2, -1, -1, 1, 2, -1, 4, 5]
    assert w["W"].tobytes() != before["W"].tobytes() and w["oW"].tobytes() != before["oW"].tobytes()
    assert ("oHT" in w) == (g["store_ht"] and g["N"] > 0)


def _plan_world(n=6, qc=8, head=0, staged=0, stopped=(), empty=(), **kw):
    geo = dict(n=n, K=2, G=8, N=4, qc=qc, R=n + max(staged, 1), Gp=40, head=head)
    geo.update(kw)
    w = sm.make_world(**geo)
    sm.stage(w, range(n, n + staged))
    sm.set_stopped(w, stopped)
    for pos in empty:           # emptied by an earlier call: stopped, no occupant
        w["occ"][pos] = -1
    w["gate"][0] = 7            # neither 0 nor 1: an untouched gate is seen
    return w


def _plan_cases():
    every = tuple(range(6))
    return {
        # name: (world, occ after, head after, done after, gate after)
        "nothing_stopped": (_plan_world(staged=4), [0, 1, 2, 3, 4, 5], 0, 0, 7),
        "all_stopped_ring_full": (_plan_world(staged=8, stopped=every),
                                  [6, 7, 8, 9, 10, 11], 6, 6, 1),
        "all_stopped_ring_empty": (_plan_world(head=5, stopped=every), [-1] * 6, 5, 6, 7),
        "ring_shorter_than_freed": (_plan_world(staged=2, stopped=(0, 2, 3, 5)),
                                    [6, 1, 7, -1, 4, -1], 2, 4, 1),
        "empty_positions_refilled": (_plan_world(staged=3, stopped=(1, 2, 4), empty=(1, 4)),
                                     [0, 6, 7, 3, 8, 5], 3, 1, 1),
        "head_at_qc_minus_2": (_plan_world(head=6, staged=4, stopped=(0, 1, 3, 5)),
                               [6, 7, 2, 8, 4, 9], 10, 4, 1),
        "head_at_3qc_plus_1": (_plan_world(head=25, staged=8, stopped=every),
                               [6, 7, 8, 9, 10, 11], 31, 6, 1),
        "state_views_at_an_offset": (_plan_world(staged=3, stopped=(0, 4, 5), p0=5, st_ld=19),
                                     [6, 1, 2, 3, 7, 8], 3, 3, 1),
    }


@pytest.mark.parametrize("chunks", [1, 32])
@pytest.mark.parametrize("case", sorted(_plan_cases()))
def test_stream_swap_plan(case, chunks):
    w, occ, head, done, gate = _plan_cases()[case]
    before = _swap_both(w, chunks, (case, chunks))
    assert w["occ"].tolist() == occ
    assert (w["head"][0], w["done"][0], w["gate"][0]) == (head, done, gate)
    if case == "nothing_stopped":
        before["plan"][:] = -1
        sm.assert_worlds_equal(w, before, case)
    if case == "head_at_qc_minus_2":        # entries 6 .. 9 came from slots 6, 7, 0, 1
        assert w["plan"][:6].tolist() == [6, 7, -1, 8, -1, 9]
        assert w["ids"].tolist() == [8, 9, -1, -1, -1, -1, 6, 7]
    if case == "empty_positions_refilled":  # 1 and 4 refilled, only 2 harvested
        assert w["plan"].tolist() == [-1, 0, 1, -1, 2, -1, -1, -1, 2, -1, -1, -1]


@pytest.mark.parametrize("chunks", [1, 32])
def test_stream_swap_scan_across_1024_positions(chunks):
    """n = 1030: free positions on both sides of position 1024 (the plan's scan runs in
    chunks of 1024), and the ring runs out inside the second chunk."""
    n = 1030
    free = [pos for pos in range(n) if (pos * 7) % 3 != 0 or pos >= 1024]
    first = sum(pos < 1024 for pos in free)
    avail = first + 3
    assert len(free) - first == 6 and first > 600
    w = sm.make_world(n=n, K=1, G=8, N=0, qc=700, R=n + avail, Gp=37, head=5)
    sm.stage(w, range(n, n + avail))
    sm.set_stopped(w, free)
    _swap_both(w, chunks, ("scan", chunks))
    assert w["head"][0] == 5 + avail and w["done"][0] == len(free)
    assert w["occ"][1024:].tolist() == [n + first, n + first + 1, n + first + 2, -1, -1, -1]
    assert w["plan"][1024:1030].tolist() == [5 + first, 6 + first, 7 + first, -1, -1, -1]


class _DeviceMirror(sm.NoMirror):
    """A device copy of the sequence's world: the host steps repeated on it, the swap by the
    kernel, and a bitwise comparison with the model's world after every pass."""
    RING = ("rW", "rHT", "rparts", "rwpl", "rsf", "rsi", "ids", "tail")

    def __init__(self, w):
        self.d = _to_device(w)
        self.compared = 0

    def staged(self, w):
        for k in self.RING:
            self.d[k].copy_(torch.from_numpy(w[k]))

    def stopped(self, cols, errs, passes):
        for c, e in zip(cols, errs):
            self.d["sf"][2, c] = e
            self.d["si"][2, c] = passes
            self.d["si"][0, c] = 0

    def swap(self, w, what):
        sm.assert_worlds_equal(_to_host(self.d), w, what + " (before)")
        ops.stream_swap(*sm.swap_views(self.d))
        torch.cuda.synchronize()

    def compare(self, w, what):
        sm.assert_worlds_equal(_to_host(self.d), w, what)
        self.compared += 1


def test_stream_swap_sequence():
    w = sm.sequence_world()
    mirror = _DeviceMirror(w)
    log = sm.run_sequence(w, mirror)
    assert mirror.compared == log["passes"] >= 4
    assert w["head"][0] == sm.SEQ_IDS - 12 > w["geo"]["qc"]         # the ring wrapped
    sm.check_sequence(_to_host(mirror.d), log)


# ---------------------------------------------------------------------------- stream_publish
def test_stream_publish_mailbox():
    box = ops.HostMailbox(width=5, slots=4)
    assert tuple(box.host.shape) == (4, 6) and (box.host == -1).all()
    mail = np.full((4, 6), -1, np.int32)
    seq_m, seq_d = np.zeros(1, np.int32), torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in range(10):
        # five counters, and at every third publish eight: truncated at the row's width
        ctr = (100 * t + np.arange(8 if t % 3 == 2 else 5)).astype(np.int32)
        ops.stream_publish(_cuda(ctr), seq_d, box)
        torch.cuda.synchronize()
        sm.publish_model(ctr, seq_m, mail)
        assert np.array_equal(box.host.numpy(), mail), t
        assert seq_d.item() == seq_m[0] == t + 1
        assert box.read(t) == ctr[:5].tolist()
        for q in range(max(0, t - 3), t):           # still live
            assert box.read(q) == mail[q % 4, 1:].tolist()
        if t >= 4:                                  # overwritten four publishes later
            assert box.read(t - 4) is None
        assert box.read(t + 1) is None              # not published yet
    # a block shorter than the row leaves the rest of the row as it was
    ops.stream_publish(_cuda(np.array([1, 2], np.int32)), seq_d, box)
    torch.cuda.synchronize()
    sm.publish_model(np.array([1, 2], np.int32), seq_m, mail)
    assert np.array_equal(box.host.numpy(), mail) and mail[10 % 4].tolist()[:3] == [10, 1, 2]


# --------------------------------------------------------------------------------- the chain
def _chain_err(i, k):
    """Error of replicate i at its k-th pass (k = 0: the initial factors)."""
    e0 = 20.0 + i % 5
    kind = i % 4
    if kind == 0:                   # falls 10 % a pass: stopped by the pass limit
        return e0 * 0.9 ** k
    if kind == 1:                   # falls once, then rises: converged at its pass 2
        return e0 * 0.9 if k == 1 else e0 * (1.0 + 0.01 * k if k else 1.0)
    if kind == 2:                   # rises at once
        return e0 * (1.0 + 0.05 * k)
    return e0 * (0.9 ** k if k <= 2 else 0.81 - 5e-5 * (k - 2))     # 5e-5 at pass 3


def _chain_stats(ids, ks, x_sq):
    lin = np.array([2.0 + 0.5 * (i % 3) for i in ids], np.float32)
    e = np.array([_chain_err(i, k) for i, k in zip(ids, ks)])
    quad = (e * e - x_sq + 2.0 * lin.astype(np.float64)).astype(np.float32)
    return lin, quad


def test_conv_update_swap_publish_chain():
    """conv_update (device pass counting, pass limit 4) -> stream_swap -> stream_publish for
    six passes on 20 positions, against the three models chained the same way."""
    n, qc, block, R, x_sq, tol, max_pass = 20, 16, 8, 44, 1000.0, 1e-4, 4
    w = sm.make_world(n=n, K=2, G=8, N=4, qc=qc, R=R, Gp=40, S=2)
    d = _to_device(w)
    box = ops.HostMailbox(width=2, slots=4)
    mail = np.full((4, 3), -1, np.int32)
    seq_m, seq_d = np.zeros(1, np.int32), torch.zeros(1, dtype=torch.int32, device="cuda")
    flags_m, fc_m = np.full((2, n), -1, np.int32), np.zeros(1, np.int32)
    flags_d = torch.full((2, n), -1, dtype=torch.int32).pin_memory()
    fc_d = torch.zeros(1, dtype=torch.int32, device="cuda")

    def conv_state(x):
        return {"err_init": x["sf"][0, :n], "err_prev": x["sf"][1, :n], "err": x["sf"][2, :n],
                "active": x["si"][0, :n], "converged": x["si"][1, :n], "n_pass": x["si"][2, :n]}

    def both_conv(lin, quad, init):
        rel = sm.conv_update_model(lin, quad, x_sq, conv_state(w), n, -1, tol, False, init=init,
                                   max_pass=max_pass, gate=w["gate"], host_flags=(flags_m, fc_m))
        ops.conv_update(_cuda(lin), _cuda(quad), x_sq, conv_state(d), n, -1, tol, False,
                        init=init, gate=d["gate"], max_pass=max_pass, host_flags=(flags_d, fc_d))
        return rel

    def compare(what):
        torch.cuda.synchronize()
        h = _to_host(d)
        floats = {k: (h.pop(k), w[k]) for k in ("sf", "osf")}
        sm.assert_worlds_equal(h, {k: v for k, v in w.items() if k not in floats}, what)
        for k, (got, want) in floats.items():
            _ulp(got, want, (what, k))
        assert np.array_equal(flags_d.numpy(), flags_m) and fc_d.item() == fc_m[0], what
        assert np.array_equal(box.host.numpy(), mail) and seq_d.item() == seq_m[0], what

    both_conv(*_chain_stats(range(n), [0] * n, x_sq), init=True)
    compare("initial error")
    next_id = n
    for p in range(1, 7):
        if next_id < R and qc - int(w["tail"][0] - w["head"][0]) >= block:
            ids = list(range(next_id, next_id + block))
            slots = [(int(w["tail"][0]) + j) % qc for j in range(block)]
            sm.stage(w, ids)
            st = sm.conv_state(block)           # staged as the init-mode step leaves them
            sm.conv_update_model(*_chain_stats(ids, [0] * block, x_sq), x_sq, st, block, 0, tol,
                                 False, init=True)
            for j, s in enumerate(slots):
                w["rsf"][:, s] = st["err"][j]
                w["rsi"][:3, s] = [1, 0, 0]
            next_id += block
            for k in _DeviceMirror.RING:
                d[k].copy_(torch.from_numpy(w[k]))
        ids = [max(int(i), 0) for i in w["occ"]]
        rel = both_conv(*_chain_stats(ids, (w["si"][2, :n] + 1).tolist(), x_sq), init=False)
        sm.check_margin(rel, tol, np.zeros(n, bool))
        ops.stream_swap(*sm.swap_views(d))
        sm.stream_swap_model(*sm.swap_views(w))
        ctr_d = torch.cat([d["done"], d["head"]])
        ops.stream_publish(ctr_d, seq_d, box)
        sm.publish_model(np.concatenate([w["done"], w["head"]]), seq_m, mail)
        compare(f"pass {p}")
        assert box.read(p - 1) == [int(w["done"][0]), int(w["head"][0])]
    assert w["done"][0] >= 20 and w["head"][0] > qc and w["si"][2, :n].max() == max_pass
    assert set(w["osi"][1, :R].tolist()) == {-21, 0, 1}     # converged and limited ones
    print(f"chain: largest ulp distance so far {_seen['ulp']}")
