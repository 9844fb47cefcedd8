"""The host models of the pass bookkeeping kernels (stream_model.py) on hand-worked cases
whose expected arrays are written out below, and ops.reference.conv_update against
conv_update_model over every mode and edge input of the GPU test (bitwise: both sides are
float64 on the CPU).  The GPU kernels are compared with these models in
test_stream_kernels_gpu.py."""
import copy

import numpy as np
import pytest
import torch

from cnmf_torch_amd.ops import reference

import stream_model as sm

NAN = float("nan")


# ------------------------------------------------------------------------------ conv_update
def test_conv_update_model_hand_worked():
    # x_sq = 25, lin = 0: err = sqrt(25 + quad)
    st = sm.conv_state(4)
    gate = np.array([5], np.int32)
    flags, ctr = np.full((2, 4), -1, np.int32), np.array([0], np.int32)
    z = np.zeros(4, np.float32)
    sm.conv_update_model(z, z, 25.0, st, 4, 0, 0.1, False, init=True, gate=gate,
                         host_flags=(flags, ctr))
    for k in ("err_init", "err_prev", "err"):
        assert st[k].tolist() == [5.0, 5.0, 5.0, 5.0]
    assert st["active"].tolist() == [1, 1, 1, 1] and st["converged"].tolist() == [0, 0, 0, 0]
    assert st["n_pass"].tolist() == [0, 0, 0, 0] and gate.tolist() == [1]
    assert flags.tolist() == [[1, 1, 1, 1], [-1, -1, -1, -1]] and ctr.tolist() == [1]
    # errors 4 (rel 0.2: goes on), 4.75 (rel 0.05 < 0.1: converged), 6 (rises: stops at
    # once, "converged"), NaN (never below tol: goes on with a NaN err_prev)
    quad = np.array([-9.0, -2.4375, 11.0, NAN], np.float32)
    rel = sm.conv_update_model(z, quad, 25.0, st, 4, 1, 0.1, False, gate=gate,
                               host_flags=(flags, ctr))
    np.testing.assert_array_equal(rel, [0.2, 0.05, -0.2, NAN])
    np.testing.assert_array_equal(st["err"], [4.0, 4.75, 6.0, NAN])
    np.testing.assert_array_equal(st["err_prev"], [4.0, 5.0, 5.0, NAN])
    assert st["err_init"].tolist() == [5.0, 5.0, 5.0, 5.0]
    assert st["active"].tolist() == [1, 0, 0, 1] and st["converged"].tolist() == [0, 1, 1, 0]
    assert st["n_pass"].tolist() == [1, 1, 1, 1] and gate.tolist() == [1]
    assert flags.tolist() == [[1, 1, 1, 1], [1, 0, 0, 1]] and ctr.tolist() == [2]
    # device counting with a limit of 2: radicand -75 clamps to err 0 (rel 0.8), the NaN
    # replicate stays NaN; both stop at the limit, unconverged; stopped ones are untouched
    quad = np.array([-100.0, 0.0, 0.0, 0.0], np.float32)
    rel = sm.conv_update_model(z, quad, 25.0, st, 4, -1, 0.1, False, max_pass=2, gate=gate,
                               host_flags=(flags, ctr))
    np.testing.assert_array_equal(rel, [0.8, NAN, NAN, NAN])
    np.testing.assert_array_equal(st["err"], [0.0, 4.75, 6.0, 5.0])
    np.testing.assert_array_equal(st["err_prev"], [4.0, 5.0, 5.0, NAN])
    assert st["active"].tolist() == [0, 0, 0, 0] and st["converged"].tolist() == [0, 1, 1, 0]
    assert st["n_pass"].tolist() == [2, 1, 1, 2] and gate.tolist() == [0]
    assert flags.tolist() == [[0, 0, 0, 0], [1, 0, 0, 1]] and ctr.tolist() == [3]
    # nothing active: only the gate, the flags slot and the counter are written
    before = copy.deepcopy(st)
    sm.conv_update_model(z, quad, 25.0, st, 4, -1, 0.1, True, max_pass=2, gate=gate,
                         host_flags=(flags, ctr))
    for k in st:
        np.testing.assert_array_equal(st[k], before[k])
    assert gate.tolist() == [0] and ctr.tolist() == [4]
    assert flags.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]


def test_conv_update_model_floor_and_final():
    # err_init = 0: the denominator is 1e-300, so any rise is an enormous negative rel
    st = sm.conv_state(2)
    z = np.zeros(2, np.float32)
    sm.conv_update_model(z, np.array([-4.0, 5.0], np.float32), 4.0, st, 2, 0, 0.0, False,
                         init=True)
    assert st["err_init"].tolist() == [0.0, 3.0]
    rel = sm.conv_update_model(z, np.array([-4.0, 0.0], np.float32), 4.0, st, 2, 1, 0.0, False)
    assert rel.tolist() == [0.0, 1.0 / 3.0]          # exactly 0 is not < tol = 0: goes on
    assert st["active"].tolist() == [1, 1]
    rel = sm.conv_update_model(z, np.array([-3.0, -3.0], np.float32), 4.0, st, 2, 7, 0.0, True)
    assert rel.tolist() == [-1.0 / 1e-300, 1.0 / 3.0]
    assert st["active"].tolist() == [0, 0] and st["converged"].tolist() == [1, 0]
    assert st["n_pass"].tolist() == [7, 7] and st["err_prev"].tolist() == [0.0, 2.0]


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("tol", [0.0, 1e-4])
@pytest.mark.parametrize("n", [1, 23, 700])
def test_reference_conv_update_matches_model(n, tol, mode):
    x_sq, lins, quads, exact = sm.conv_inputs(n)
    st_m = sm.conv_state(n)
    st_r = {k: torch.from_numpy(v.copy()) for k, v in st_m.items()}
    stopped_converged = np.zeros(n, bool)
    for p, (pass_idx, final, init, max_pass) in enumerate(sm.conv_protocol(mode)):
        rel = sm.conv_update_model(lins[p], quads[p], x_sq, st_m, n, pass_idx, tol, final,
                                   init=init, max_pass=max_pass)
        reference.conv_update(torch.from_numpy(lins[p]), torch.from_numpy(quads[p]), x_sq, st_r,
                              n, pass_idx, tol, final, init=init, max_pass=max_pass)
        if not init:
            sm.check_margin(rel, tol, exact[p])
        for k in st_m:
            got = st_r[k].numpy()
            assert got.dtype == st_m[k].dtype
            assert got.tobytes() == st_m[k].tobytes(), (k, p, got, st_m[k])
        stopped_converged |= st_m["converged"] != 0
    assert not st_m["active"].any()
    kinds = np.array([sm.CONV_KINDS[r % len(sm.CONV_KINDS)] for r in range(n)])
    # what the inputs are for: non-finite statistics never converge, a rise always does,
    # an exact repeat converges only under a positive tol
    for kind in ("lin_nan", "quad_nan", "nan_init"):
        assert not stopped_converged[kinds == kind].any()
    for kind in ("rise", "neg", "zero_init", "lin_inf"):
        assert stopped_converged[kinds == kind].all()
    for kind in ("repeat", "slow"):
        assert (stopped_converged[kinds == kind] == (tol > 0)).all()
    assert not stopped_converged[kinds == "fall"].any()


# ------------------------------------------------------------------------------ stream_swap
def _tiny(n, occ, active, qc, head, slot_ids, tail, R):
    """K = 1, G = 2, N = 1, S = 1, Gp = 1.  Replicate i carries W row [10 i, 10 i + 1], HT
    row [100 + i], parts 200 + i, plane p value 1000 (p + 1) + i, sf column [i + .25,
    i + .5, i + .75], si column [active, i, 20 + i, 30 + i, 40 + i].  Position p of the batch
    holds replicate 50 + p when occ[p] is -1 (stale contents).  Store rows are sentinels
    (-1), replicate i's row is i."""
    f32, i32 = np.float32, np.int32

    def fill(ids, act):
        m = len(ids)
        d = {"W": np.zeros((m, 2), f32), "HT": np.zeros((m, 1), f32),
             "parts": np.zeros((m, 1, 1, 1), f32), "wpl": np.zeros((3, m, 1), np.int16),
             "sf": np.zeros((3, m)), "si": np.zeros((5, m), i32)}
        for p, i in enumerate(ids):
            d["W"][p] = [10 * i, 10 * i + 1]
            d["HT"][p] = [100 + i]
            d["parts"][p] = 200 + i
            d["wpl"][:, p, 0] = [1000 + i, 2000 + i, 3000 + i]
            d["sf"][:, p] = [i + .25, i + .5, i + .75]
            d["si"][:, p] = [act[p], i, 20 + i, 30 + i, 40 + i]
        return d

    b = fill([o if o >= 0 else 50 + p for p, o in enumerate(occ)], active)
    r = fill(slot_ids, [1] * qc)
    grp = {"n": n, "K": 1, "active": b["si"][0], "occ": np.array(occ, i32),
           "plan": np.full(2 * n, -3, i32), "W": b["W"], "HT": b["HT"], "parts": b["parts"],
           "wpl": b["wpl"]}
    ring = {"qc": qc, "head": np.array([head], i32), "tail": np.array([tail], i32),
            "ids": np.array(slot_ids, i32), "W": r["W"], "HT": r["HT"], "sf": r["sf"],
            "si": r["si"], "parts": r["parts"], "wpl": r["wpl"]}
    store = {"offs": np.arange(R, dtype=np.int64), "W": np.full((R, 2), -1, f32),
             "HT": np.full((R, 1), -1, f32), "sf": np.full((3, R), -1.0),
             "si": np.full((5, R), -1, i32), "done": np.array([0], i32)}
    return grp, ring, store, (b["sf"], b["si"]), np.array([0], i32)


def test_swap_model_short_ring_and_same_position():
    # positions 1, 2, 3 stopped; the ring holds two entries (replicates 4, 5 in slots
    # 0, 1): 1 and 2 are harvested AND refilled in this call, 3 is harvested and left empty
    grp, ring, store, (sf, si), gate = _tiny(4, [0, 1, 2, 3], [1, 0, 0, 0], qc=4, head=0,
                                             slot_ids=[4, 5, 6, 7], tail=2, R=8)
    ring_before = copy.deepcopy(ring)
    sm.stream_swap_model(grp, ring, store, (sf, si), gate)
    assert grp["plan"].tolist() == [-1, 0, 1, -1, -1, 1, 2, 3]
    assert grp["occ"].tolist() == [0, 4, 5, -1]
    assert ring["head"].tolist() == [2] and store["done"].tolist() == [3]
    assert gate.tolist() == [1]
    assert grp["W"].tolist() == [[0, 1], [40, 41], [50, 51], [30, 31]]
    assert grp["HT"].tolist() == [[100], [104], [105], [103]]
    assert grp["parts"].reshape(-1).tolist() == [200, 204, 205, 203]
    assert grp["wpl"][:, :, 0].tolist() == [[1000, 1004, 1005, 1003], [2000, 2004, 2005, 2003],
                                            [3000, 3004, 3005, 3003]]
    assert sf.tolist() == [[.25, 4.25, 5.25, 3.25], [.5, 4.5, 5.5, 3.5], [.75, 4.75, 5.75, 3.75]]
    assert si.tolist() == [[1, 1, 1, 0], [0, 4, 5, 3], [20, 24, 25, 23], [30, 34, 35, 33],
                           [40, 44, 45, 43]]
    # the store holds the OLD contents of positions 1, 2, 3 in rows 1, 2, 3
    assert store["W"].tolist() == [[-1, -1], [10, 11], [20, 21], [30, 31]] + [[-1, -1]] * 4
    assert store["HT"].reshape(-1).tolist() == [-1, 101, 102, 103, -1, -1, -1, -1]
    assert store["sf"].tolist() == [[-1, 1.25, 2.25, 3.25, -1, -1, -1, -1],
                                    [-1, 1.5, 2.5, 3.5, -1, -1, -1, -1],
                                    [-1, 1.75, 2.75, 3.75, -1, -1, -1, -1]]
    assert store["si"].tolist() == [[-1, 0, 0, 0, -1, -1, -1, -1], [-1, 1, 2, 3, -1, -1, -1, -1],
                                    [-1, 21, 22, 23, -1, -1, -1, -1],
                                    [-1, 31, 32, 33, -1, -1, -1, -1],
                                    [-1, 41, 42, 43, -1, -1, -1, -1]]
    for k in ("ids", "W", "HT", "sf", "si", "parts", "wpl", "tail"):
        np.testing.assert_array_equal(ring[k], ring_before[k])


def test_swap_model_wrapped_ring_and_empty_position():
    # head = 7 of a ring of 4 (the head has passed the capacity), two entries published:
    # entries 7, 8 sit in slots 3, 0 (replicates 10, 11; slots 1, 2 are stale).  Position 0
    # (replicate 6) stopped; position 1 is empty since an earlier call (occ -1, stale
    # contents of "replicate 51"): refilled, not harvested again; position 2 is active
    grp, ring, store, (sf, si), gate = _tiny(3, [6, -1, 2], [0, 0, 1], qc=4, head=7,
                                             slot_ids=[11, 8, 9, 10], tail=9, R=12)
    gate[0] = 0
    store["done"][0] = 5
    sm.stream_swap_model(grp, ring, store, (sf, si), gate)
    assert grp["plan"].tolist() == [7, 8, -1, 6, -1, -1]
    assert grp["occ"].tolist() == [10, 11, 2]
    assert ring["head"].tolist() == [9] and store["done"].tolist() == [6]
    assert gate.tolist() == [1]
    assert grp["W"].tolist() == [[100, 101], [110, 111], [20, 21]]
    assert grp["HT"].reshape(-1).tolist() == [110, 111, 102]
    assert grp["parts"].reshape(-1).tolist() == [210, 211, 202]
    assert grp["wpl"][:, :, 0].tolist() == [[1010, 1011, 1002], [2010, 2011, 2002],
                                            [3010, 3011, 3002]]
    assert sf.tolist() == [[10.25, 11.25, 2.25], [10.5, 11.5, 2.5], [10.75, 11.75, 2.75]]
    assert si.tolist() == [[1, 1, 1], [10, 11, 2], [30, 31, 22], [40, 41, 32], [50, 51, 42]]
    w = [[-1.0, -1.0]] * 12
    w[6] = [60.0, 61.0]
    assert store["W"].tolist() == w
    assert store["HT"].reshape(-1).tolist() == [-1] * 6 + [106] + [-1] * 5
    assert store["sf"][:, 6].tolist() == [6.25, 6.5, 6.75]
    assert store["si"][:, 6].tolist() == [0, 6, 26, 36, 46]
    assert (np.delete(store["sf"], 6, axis=1) == -1).all()
    assert (np.delete(store["si"], 6, axis=1) == -1).all()


def test_swap_model_nothing_to_do_and_empty_ring():
    # nothing stopped: only the plan is written (all -1); the gate keeps its value
    grp, ring, store, st, gate = _tiny(2, [0, 1], [1, 1], qc=2, head=0, slot_ids=[2, 3],
                                       tail=2, R=4)
    gate[0] = 0
    keep = copy.deepcopy((grp, ring, store, st))
    sm.stream_swap_model(grp, ring, store, st, gate)
    assert grp["plan"].tolist() == [-1, -1, -1, -1] and gate.tolist() == [0]
    grp["plan"][:] = -3
    for a, b in zip((grp, ring, store), keep[:3]):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
    # ring consumed (tail == head, both past the capacity): harvest only, the gate stays 0,
    # store HT absent
    grp, ring, store, (sf, si), gate = _tiny(2, [0, 1], [0, 1], qc=2, head=5, slot_ids=[2, 3],
                                             tail=5, R=4)
    store["HT"] = None
    sm.stream_swap_model(grp, ring, store, (sf, si), gate)
    assert grp["plan"].tolist() == [-1, -1, 0, -1] and grp["occ"].tolist() == [-1, 1]
    assert ring["head"].tolist() == [5] and store["done"].tolist() == [1]
    assert gate.tolist() == [0]
    assert grp["W"].tolist() == [[0, 1], [10, 11]] and si[0].tolist() == [0, 1]
    assert store["W"].tolist() == [[0, 1], [-1, -1], [-1, -1], [-1, -1]]
    assert store["si"][:, 0].tolist() == [0, 0, 20, 30, 40]


def test_publish_model_hand_worked():
    mail = np.full((2, 3), -1, np.int32)
    seq = np.array([0], np.int32)
    sm.publish_model(np.array([7, 8, 9], np.int32), seq, mail)      # truncated at width
    assert mail.tolist() == [[0, 7, 8], [-1, -1, -1]] and seq.tolist() == [1]
    sm.publish_model(np.array([5], np.int32), seq, mail)            # shorter: rest kept
    assert mail.tolist() == [[0, 7, 8], [1, 5, -1]] and seq.tolist() == [2]
    sm.publish_model(np.array([3, 4], np.int32), seq, mail)         # row 0 overwritten
    assert mail.tolist() == [[2, 3, 4], [1, 5, -1]] and seq.tolist() == [3]


# ------------------------------------------------------------------- worlds and the sequence
def test_world_views_alias_their_buffers():
    w = sm.make_world(n=3, K=2, G=5, N=3, qc=4, R=9, ldw=7, ldh=4, pl_ld=9, Gp=6, w_off=1,
                      ow_off=1, p0=2, st_ld=8)
    grp, ring, store, (sf, si), _ = sm.swap_views(w)
    rep = sm.replicate(w["geo"], 2)
    np.testing.assert_array_equal(grp["W"][4:6], rep["W"])
    assert w["W"][1 + 4 * 7] == rep["W"][0, 0] and w["W"][0] == -7.0 and w["W"][1 + 5] == -7.0
    assert grp["active"].tolist() == [1, 1, 1] and w["si"][0].tolist()[:2] == [-11, -11]
    assert store["offs"].tolist() == [16, 14, 12, 10, 8, 6, 4, 2, 0]
    sm.stage(w, [3, 4])
    assert w["tail"].tolist() == [2] and w["ids"].tolist() == [3, 4, -1, -1]
    np.testing.assert_array_equal(ring["W"][2:4], sm.replicate(w["geo"], 4)["W"])
    sm.set_stopped(w, [1])
    before = copy.deepcopy(w)
    sm.stream_swap_model(*sm.swap_views(w))
    assert w["occ"].tolist() == [0, 3, 2] and w["done"].tolist() == [1]
    # padding between the columns and the pitch, and in front of the misaligned bases
    pad = np.ones(w["W"].shape, bool)
    pad[(1 + np.arange(6)[:, None] * 7 + np.arange(5)).reshape(-1)] = False
    np.testing.assert_array_equal(w["W"][pad], before["W"][pad])
    np.testing.assert_array_equal(store["W"][14:16], sm.replicate(w["geo"], 1)["W"])
    with pytest.raises(AssertionError):
        sm.assert_worlds_equal(w, before)
    sm.assert_worlds_equal(w, copy.deepcopy(w))


def test_sequence_on_the_model_alone():
    w = sm.sequence_world()
    log = sm.run_sequence(w)
    assert log["passes"] >= 4
    sm.check_sequence(w, log)
