"""Plain host models of the pass bookkeeping kernels (conv.hip conv_update_kernel,
stream.hip stream_plan_kernel / stream_copy_kernel / stream_publish_kernel), written from
their specification with numpy arrays and Python loops only, and the inputs the tests of
those kernels share (test_stream_model_cpu.py, test_stream_kernels_gpu.py).

Every model works in place on numpy arrays laid out like the arguments of the matching
``ops`` wrapper, views included: a test builds one set of base buffers, hands views of
them to the model and views of a device copy to the kernel, and compares whole buffers."""
import numpy as np

# ------------------------------------------------------------------------------ conv_update


def conv_update_model(lin, quad, x_sq, state, n, pass_idx, tol, final, init=False,
                      max_pass=0, gate=None, host_flags=None):
    """The outer stop rule, one replicate at a time.  ``state``: float64 err_init /
    err_prev / err and int32 active / converged / n_pass arrays; ``gate``: int32 [1] or
    None; ``host_flags``: (int32 (2, n) flags, int32 [1] launch counter) or None.
    Returns the relative improvement evaluated per replicate (NaN where none was)."""
    rel_out = np.full(n, np.nan)
    if n <= 0:
        return rel_out
    any_active = 0
    with np.errstate(all="ignore"):
        for r in range(n):
            rad = np.float64(x_sq) - np.float64(2.0) * np.float64(lin[r]) + np.float64(quad[r])
            if rad < 0.0:           # a NaN radicand is not below 0: it stays NaN
                rad = np.float64(0.0)
            e = np.sqrt(rad)
            if init:
                state["err_init"][r] = state["err_prev"][r] = state["err"][r] = e
                state["active"][r] = 1
                state["converged"][r] = 0
                state["n_pass"][r] = 0
                any_active = 1
                continue
            if state["active"][r] == 0:
                continue
            state["err"][r] = e
            n_pass = pass_idx if pass_idx >= 0 else int(state["n_pass"][r]) + 1
            state["n_pass"][r] = n_pass
            denom = state["err_init"][r]
            if denom < 1e-300:      # (NaN stays)
                denom = np.float64(1e-300)
            rel = (state["err_prev"][r] - e) / denom
            rel_out[r] = rel
            if rel < tol:
                state["active"][r] = 0
                state["converged"][r] = 1
            elif final or (max_pass > 0 and n_pass >= max_pass):
                state["active"][r] = 0
            else:
                state["err_prev"][r] = e
                any_active = 1
    if gate is not None:
        gate[0] = any_active
    if host_flags is not None:
        flags, counter = host_flags
        flags[int(counter[0]) & 1, :n] = state["active"][:n]
        counter[0] += 1
    return rel_out


CONV_KINDS = ("fall", "rise", "repeat", "slow", "neg", "zero_init", "lin_nan", "quad_nan",
              "lin_inf", "nan_init")
CONV_PASSES = 5
CONV_X_SQ = 1000.0


def _conv_err(kind: str, r: int, p: int):
    """Target error of replicate r (of ``kind``) at pass p (0 = initial factors), or a
    marker string for the non-finite / clamped statistics."""
    e0 = 20.0 + (r % 7) + 0.125 * (r % 3)
    fall = e0 * (0.9 - 0.01 * (r % 4)) ** p                 # >= 6 % of e0 per pass here
    if kind == "fall":
        return fall
    if kind == "rise":                                      # falls once, then rises
        return fall if p <= 1 else e0 * (0.9 + 0.02 * p)
    if kind == "repeat":                                    # pass 2 repeats pass 1's inputs
        return fall if p <= 1 else (e0 * (0.9 - 0.01 * (r % 4)) if p == 2 else
                                    e0 * 0.7 * 0.9 ** (p - 2))
    if kind == "slow":                                      # 5e-5 of e0 at pass 3
        return fall if p <= 2 else e0 * ((0.9 - 0.01 * (r % 4)) ** 2 - 5e-5 * (p - 2))
    if kind == "neg":                                       # radicand below 0 at pass 2
        return "neg" if p == 2 else (fall if p < 2 else e0 * 0.5)
    if kind == "zero_init":                                 # 0, 0 again, then up
        return 0.0 if p <= 1 else 3.0 + p
    if kind == "lin_nan":
        return fall if p <= 1 else ("lin_nan" if p <= 3 else fall)
    if kind == "quad_nan":
        return "quad_nan"
    if kind == "lin_inf":
        return "lin_inf" if p == 1 else (e0 if p == 0 else 4.0 + p)
    if kind == "nan_init":
        return "quad_nan" if p == 0 else fall
    raise ValueError(kind)


def conv_inputs(n: int):
    """x_sq, the float32 (lin, quad) of the initial factors and of CONV_PASSES passes for
    n replicates cycling through CONV_KINDS, and per pass the mask of replicates whose
    inputs repeat the pass before (there the relative improvement is exactly 0)."""
    lins, quads, exact = [], [], []
    for p in range(CONV_PASSES + 1):
        lin = np.zeros(n, dtype=np.float32)
        quad = np.zeros(n, dtype=np.float32)
        ex = np.zeros(n, dtype=bool)
        for r in range(n):
            kind = CONV_KINDS[r % len(CONV_KINDS)]
            t = _conv_err(kind, r, p)
            lin[r] = np.float32(3.0 + 0.25 * (r % 5))
            if t == "neg":
                quad[r] = np.float32(-CONV_X_SQ - 50.0)
            elif t == "lin_nan":
                lin[r] = np.float32(np.nan)
            elif t == "quad_nan":
                quad[r] = np.float32(np.nan)
            elif t == "lin_inf":
                lin[r] = np.float32(np.inf)
            else:
                quad[r] = np.float32(t * t - CONV_X_SQ + 2.0 * float(lin[r]))
            if p >= 1 and lin[r] == lins[-1][r] and quad[r] == quads[-1][r]:
                ex[r] = True
        lins.append(lin)
        quads.append(quad)
        exact.append(ex)
    return CONV_X_SQ, lins, quads, exact


def conv_state(n: int):
    """Fresh conv_update state of n replicates (sentinels: init mode overwrites all)."""
    return {"err_init": np.full(n, -1.0), "err_prev": np.full(n, -2.0), "err": np.full(n, -3.0),
            "active": np.full(n, 7, dtype=np.int32), "converged": np.full(n, 8, dtype=np.int32),
            "n_pass": np.full(n, 9, dtype=np.int32)}


def conv_protocol(mode: str):
    """[(pass_idx, final, init, max_pass)] of the launches of one run: the initial error,
    then CONV_PASSES passes counted by the host ("host": final on the last) or on the
    device with a pass limit of 3 ("device": the last two find nothing active)."""
    if mode == "host":
        return [(0, False, True, 0)] + [(p, p == CONV_PASSES, False, 0)
                                        for p in range(1, CONV_PASSES + 1)]
    return [(0, False, True, 3)] + [(-1, False, False, 3)] * CONV_PASSES


def check_margin(rel, tol, exact, min_gap=1e-9):
    """Every evaluated relative improvement is NaN, exactly 0 where the inputs repeat, or
    further than ``min_gap`` from ``tol``: no stop decision rides on the last bits."""
    for r, v in enumerate(rel):
        if np.isnan(v) or (exact[r] and v == 0.0):
            continue
        assert abs(v - tol) > min_gap, (r, v, tol)


def ulp_distance(a, b):
    """Largest distance in units in the last place between float64 arrays of equal
    NaN-ness and sign (asserted); NaN pairs count 0."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (a, b)
    assert np.array_equal(np.signbit(a[~na]), np.signbit(b[~nb]))
    d = np.abs(a[~na].view(np.int64) - b[~nb].view(np.int64))
    return int(d.max()) if d.size else 0


# ------------------------------------------------------------------------------ stream_swap


def stream_swap_model(grp, ring, store, state, gate):
    """Harvest the stopped replicates of a group, then place staged ones (numpy arrays of
    the layout of the ops.stream_swap arguments; in place)."""
    n, K = int(grp["n"]), int(grp["K"])
    if n <= 0:
        return
    sf, si = state
    active, occ, plan = grp["active"], grp["occ"], grp["plan"]
    qc = int(ring["qc"])
    head, tail = int(ring["head"][0]), int(ring["tail"][0])
    avail = max(0, tail - head)
    free = [pos for pos in range(n) if active[pos] == 0]
    placed, harvested = {}, {}
    for j, pos in enumerate(free):
        if occ[pos] >= 0:
            harvested[pos] = int(occ[pos])
        if j < avail:
            placed[pos] = head + j
    for pos in range(n):
        plan[pos] = placed.get(pos, -1)
        plan[n + pos] = harvested.get(pos, -1)
    for pos in free:
        occ[pos] = ring["ids"][placed[pos] % qc] if pos in placed else -1
    ring["head"][0] = head + len(placed)
    store["done"][0] += len(harvested)
    if placed:
        gate[0] = 1
    has_ht = grp["HT"].shape[1] > 0
    # the old contents of every stopped position, before anything is placed
    for pos, h in harvested.items():
        o = int(store["offs"][h])
        for k in range(K):
            store["W"][o + k, :] = grp["W"][pos * K + k, :]
            if store["HT"] is not None:
                store["HT"][o + k, :] = grp["HT"][pos * K + k, :]
        for t in range(3):
            store["sf"][t, h] = sf[t, pos]
        for t in range(5):
            store["si"][t, h] = si[t, pos]
    for pos, e in placed.items():
        s = e % qc
        for k in range(K):
            grp["W"][pos * K + k, :] = ring["W"][s * K + k, :]
            if has_ht:
                grp["HT"][pos * K + k, :] = ring["HT"][s * K + k, :]
            for pl in range(3):
                grp["wpl"][pl, pos * K + k, :] = ring["wpl"][pl, s * K + k, :]
        grp["parts"][pos] = ring["parts"][s]
        for t in range(3):
            sf[t, pos] = ring["sf"][t, s]
        for t in range(5):
            si[t, pos] = ring["si"][t, s]


def publish_model(ctr, seq, mail):
    """Row seq % slots of the (slots, width) mailbox gets [seq, ctr[0 .. width-2]]."""
    slots, width = mail.shape
    s = int(seq[0])
    m = min(len(ctr), width - 1)
    mail[s % slots, 0] = s
    mail[s % slots, 1:1 + m] = ctr[:m]
    seq[0] = s + 1


# --------------------------------------------------------------- stream_swap test worlds
#
# A world is a dict of BASE buffers (flat or plainly shaped numpy arrays) plus its
# geometry under "geo".  swap_views() cuts the wrapper's argument views out of the base
# buffers by basic slicing and as_strided, which numpy arrays and torch tensors share:
# the same function serves the model (numpy) and the kernel (a device copy).

_PAD = 4        # spare elements behind every strided matrix


def _rows(buf, off, rows, ld, cols):
    """(rows, cols) view at row pitch ld of the flat buffer, starting at element off."""
    if isinstance(buf, np.ndarray):
        if cols == 0:
            return np.zeros((rows, 0), dtype=buf.dtype)
        isz = buf.itemsize
        return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, cols),
                                               strides=(ld * isz, isz))
    if cols == 0:
        return buf.new_zeros((rows, 0))
    return buf.as_strided((rows, cols), (ld, 1), off)


def replicate(geo, i):
    """Everything replicate id i carries, from its id alone: float32-exact values naming
    (id, row, column), so a row that lands anywhere else is seen."""
    K, G, N, S, Gp = geo["K"], geo["G"], geo["N"], geo["S"], geo["Gp"]
    kk, cc = np.meshgrid(np.arange(K), np.arange(G), indexing="ij")
    W = (((i * 8 + kk) * 256 + cc) + 0.25).astype(np.float32)
    kk, cc = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    HT = (((i * 8 + kk) * 256 + cc) + 0.5).astype(np.float32)
    parts = (i * 1024 + np.arange(S * K * K) + 0.125).astype(np.float32).reshape(S, K, K)
    pl, kk, cc = np.meshgrid(np.arange(3), np.arange(K), np.arange(Gp), indexing="ij")
    wpl = (((i * 8 + kk) * 131 + cc * 3 + pl) & 0xFFFF).astype(np.uint16).view(np.int16)
    sf = np.array([i + 0.25, i + 0.5, i + 0.75])
    si = np.array([1, 0, i * 4 + 1, i * 4 + 2, i * 4 + 3], dtype=np.int32)
    return {"W": W, "HT": HT, "parts": parts, "wpl": wpl, "sf": sf, "si": si}


def make_world(n, K, G, N, qc, R, S=1, Gp=64, ldw=None, ldh=None, pl_ld=None, w_off=0,
               ow_off=0, store_ht=True, p0=0, st_ld=None, head=0):
    """Base buffers of a group of n positions holding replicates 0 .. n-1 (all active),
    an empty ring of qc slots with ``head`` entries consumed, and an empty store of R
    replicates whose rows run in reverse id order.  Pitches default to the columns;
    ``w_off`` / ``ow_off`` start the batch / store spectra that many elements into their
    buffer; the state tables have ``st_ld`` columns with the group at column ``p0``."""
    assert K <= 8 and max(G, N) <= 256 and R * 8 * 256 < 2 ** 22
    ldw = G if ldw is None else ldw
    ldh = max(N, 1) if ldh is None else ldh
    pl_ld = Gp if pl_ld is None else pl_ld
    st_ld = p0 + n + 3 if st_ld is None else st_ld
    geo = dict(n=n, K=K, G=G, N=N, qc=qc, R=R, S=S, Gp=Gp, ldw=ldw, ldh=ldh, pl_ld=pl_ld,
               w_off=w_off, ow_off=ow_off, store_ht=store_ht, p0=p0, st_ld=st_ld)
    f32, i32 = np.float32, np.int32
    w = {"geo": geo,
         "W": np.full(w_off + n * K * ldw + _PAD, -7.0, f32),
         "HT": np.full(n * K * ldh + _PAD, -8.0, f32),
         "parts": np.zeros((n, S, K, K), f32),
         "wpl": np.full((3, n * K + 2, pl_ld), -9, np.int16),
         "sf": np.full((3, st_ld), -10.0), "si": np.full((5, st_ld), -11, i32),
         "occ": np.arange(n, dtype=i32), "plan": np.full(2 * n, -3, i32),
         "rW": np.full(qc * K * ldw + _PAD, -12.0, f32),
         "rHT": np.full(qc * K * ldh + _PAD, -13.0, f32),
         "rparts": np.full((qc, S, K, K), -14.0, f32),
         "rwpl": np.full((3, qc * K, pl_ld), -15, np.int16),
         "rsf": np.full((3, qc), -16.0), "rsi": np.full((5, qc), -17, i32),
         "ids": np.full(qc, -1, i32),
         "head": np.array([head], i32), "tail": np.array([head], i32),
         "offs": ((R - 1 - np.arange(R)) * K).astype(np.int64),
         "oW": np.full(ow_off + R * K * ldw + _PAD, -18.0, f32),
         "osf": np.full((3, R + 2), -20.0), "osi": np.full((5, R + 1), -21, i32),
         "done": np.zeros(1, i32), "gate": np.zeros(1, i32)}
    if store_ht and N > 0:
        w["oHT"] = np.full(R * K * ldh + _PAD, -19.0, f32)
    grp, _, _, (sf, si), _ = swap_views(w)
    for pos in range(n):
        rep = replicate(geo, pos)
        grp["W"][pos * K:(pos + 1) * K] = rep["W"]
        if N > 0:
            grp["HT"][pos * K:(pos + 1) * K] = rep["HT"]
        grp["parts"][pos] = rep["parts"]
        grp["wpl"][:, pos * K:(pos + 1) * K] = rep["wpl"]
        sf[:, pos] = rep["sf"]
        si[:, pos] = rep["si"]
    return w


def swap_views(w):
    """(grp, ring, store, state, gate) of ops.stream_swap / stream_swap_model over the base
    buffers of a world (numpy arrays, or torch tensors of the same shapes)."""
    g = w["geo"]
    n, K, G, N, qc, R = g["n"], g["K"], g["G"], g["N"], g["qc"], g["R"]
    sf, si = w["sf"][:, g["p0"]:], w["si"][:, g["p0"]:]
    grp = {"n": n, "K": K, "active": w["si"][0, g["p0"]:g["p0"] + n], "occ": w["occ"],
           "plan": w["plan"], "W": _rows(w["W"], g["w_off"], n * K, g["ldw"], G),
           "HT": _rows(w["HT"], 0, n * K, g["ldh"], N), "parts": w["parts"],
           "wpl": w["wpl"][:, :, :g["Gp"]]}
    ring = {"qc": qc, "head": w["head"], "tail": w["tail"], "ids": w["ids"],
            "W": _rows(w["rW"], 0, qc * K, g["ldw"], G),
            "HT": _rows(w["rHT"], 0, qc * K, g["ldh"], N), "sf": w["rsf"], "si": w["rsi"],
            "parts": w["rparts"], "wpl": w["rwpl"][:, :, :g["Gp"]]}
    store = {"offs": w["offs"], "W": _rows(w["oW"], g["ow_off"], R * K, g["ldw"], G),
             "HT": _rows(w["oHT"], 0, R * K, g["ldh"], N) if "oHT" in w else None,
             "sf": w["osf"][:, :R], "si": w["osi"][:, :R], "done": w["done"]}
    return grp, ring, store, (sf, si), w["gate"]


def stage(w, ids):
    """Write replicates ``ids`` into the ring slots after the last published entry and
    raise the tail (numpy world)."""
    g = w["geo"]
    K, qc = g["K"], g["qc"]
    _, ring, _, _, _ = swap_views(w)
    for i in ids:
        s = int(w["tail"][0]) % qc
        rep = replicate(g, int(i))
        ring["W"][s * K:(s + 1) * K] = rep["W"]
        if g["N"] > 0:
            ring["HT"][s * K:(s + 1) * K] = rep["HT"]
        ring["parts"][s] = rep["parts"]
        ring["wpl"][:, s * K:(s + 1) * K] = rep["wpl"]
        ring["sf"][:, s] = rep["sf"]
        ring["si"][:, s] = rep["si"]
        ring["ids"][s] = i
        w["tail"][0] += 1


def set_stopped(w, positions):
    """Clear the active flags of ``positions`` (numpy world)."""
    g = w["geo"]
    for pos in positions:
        w["si"][0, g["p0"] + pos] = 0


def world_buffers(w):
    return [k for k in w if k != "geo"]


def assert_worlds_equal(a, b, what=""):
    """Every base buffer of world ``a`` equals ``b``'s bit for bit (numpy worlds)."""
    for k in world_buffers(a):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        if x.tobytes() != y.tobytes():
            bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[x.itemsize]
            bad = np.flatnonzero(x.reshape(-1).view(bits) != y.reshape(-1).view(bits))
            raise AssertionError(f"{what}: buffer {k} differs at {bad.size} elements, first "
                                 f"{bad[:8].tolist()}: {x.reshape(-1)[bad[:8]].tolist()} vs "
                                 f"{y.reshape(-1)[bad[:8]].tolist()}")


# ------------------------------------------------------------------------------ a sequence
SEQ_IDS = 40


def sequence_world():
    """K = 5, 12 positions, a ring of 24, 40 replicate ids; pitches wider than the columns."""
    return make_world(n=12, K=5, G=20, N=12, qc=24, R=SEQ_IDS, S=2, Gp=40, ldw=24, ldh=16,
                      pl_ld=48)


class NoMirror:
    """What run_sequence tells a second copy of the world (a device copy overrides these)."""

    def staged(self, w):
        pass

    def stopped(self, cols, errs, passes):
        pass

    def swap(self, w, what):
        pass

    def compare(self, w, what):
        pass


def run_sequence(w, mirror=None, block=12, seed=5):
    """Streaming passes on the numpy world ``w`` until every id is harvested.  Each pass:
    stage the next block of waiting ids into slots tail % qc when the ring has a block of
    room, stop a pseudo-random subset of the active positions (each records its pass and an
    error in its state columns first), let ``mirror`` do the same and swap, then swap on the
    model and let ``mirror`` compare.  Returns the harvest log: per id how often it was harvested and what its rows
    held when it stopped."""
    mirror = mirror or NoMirror()
    g = w["geo"]
    n, K, qc, p0 = g["n"], g["K"], g["qc"], g["p0"]
    grp, ring, store, (sf, si), gate = swap_views(w)
    rng = np.random.default_rng(seed)
    next_id, passes = n, 0
    log = {"count": {}, "held": {}, "passes": 0}
    while int(w["done"][0]) < SEQ_IDS:
        passes += 1
        assert passes < 100
        if next_id < SEQ_IDS and qc - (int(w["tail"][0]) - int(w["head"][0])) >= block:
            ids = list(range(next_id, min(SEQ_IDS, next_id + block)))
            assert int(w["tail"][0]) % qc + len(ids) <= qc
            stage(w, ids)
            next_id = ids[-1] + 1
            mirror.staged(w)
        act = [pos for pos in range(n) if grp["active"][pos] != 0]
        stop = [pos for pos in act if rng.random() < 0.4] or act[:1]
        errs = [passes + int(grp["occ"][pos]) / 64.0 for pos in stop]
        for pos, e in zip(stop, errs):
            sf[2, pos] = e
            si[2, pos] = passes
            si[0, pos] = 0
            i = int(grp["occ"][pos])
            assert i >= 0 and i not in log["held"]
            log["held"][i] = {"W": grp["W"][pos * K:(pos + 1) * K].copy(),
                              "HT": grp["HT"][pos * K:(pos + 1) * K].copy(),
                              "sf": sf[:, pos].copy(), "si": si[:, pos].copy()}
        mirror.stopped([p0 + pos for pos in stop], errs, passes)
        mirror.swap(w, f"pass {passes}")
        stream_swap_model(grp, ring, store, (sf, si), gate)
        mirror.compare(w, f"pass {passes}")
        for i in grp["plan"][n:2 * n]:
            if i >= 0:
                log["count"][int(i)] = log["count"].get(int(i), 0) + 1
    log["passes"] = passes
    return log


def check_sequence(w, log):
    """Every id was harvested exactly once, and its store rows hold what it had when it
    stopped (``w``: a numpy world after run_sequence, the model's or a device copy)."""
    g = w["geo"]
    K = g["K"]
    _, _, store, _, _ = swap_views(w)
    assert log["count"] == {i: 1 for i in range(SEQ_IDS)}, log["count"]
    assert int(w["done"][0]) == SEQ_IDS and (w["occ"] == -1).all()
    for i in range(SEQ_IDS):
        o = int(store["offs"][i])
        held = log["held"][i]
        assert held["si"][0] == 0 and held["si"][2] >= 1
        np.testing.assert_array_equal(held["W"], replicate(g, i)["W"])
        assert store["W"][o:o + K].tobytes() == held["W"].tobytes(), i
        assert store["HT"][o:o + K].tobytes() == held["HT"].tobytes(), i
        assert store["sf"][:, i].tobytes() == held["sf"].tobytes(), i
        assert store["si"][:, i].tobytes() == held["si"].tobytes(), i
