"""PyTorch reference implementations of the native ops (CPU path + test oracle).

They implement exactly the contract of the HIP kernels (csrc/kernels/*.hip) in
vectorised torch, in whatever dtype they are given (float64 for the oracle).
"""
from __future__ import annotations

import numpy as np
import torch

from ..utils.rng import philox_matrix


def _objective(X, N, G, l1, l2):
    """Block objective per replicate: sum x^T G x - 2 n.x + 2 l1 |x|_1 + l2 |x|^2."""
    q = (X * (torch.bmm(G, X) + l2 * X)).sum(dim=(1, 2))
    lin = (X * (N - l1)).sum(dim=(1, 2))
    return q - 2.0 * lin


def _step(algo, Xa, Na, Ga, l1_den, l2, eps):
    K = Xa.shape[1]
    if algo == 0:
        den = torch.bmm(Ga, Xa) + l2 * Xa + l1_den
        return torch.where(den < eps, torch.zeros_like(Xa), Xa * (Na / den))
    Xn = Xa.clone()
    for k in range(K):
        gx = torch.bmm(Ga[:, k:k + 1, :], Xn).squeeze(1)
        diag = (Ga[:, k, k] + l2).unsqueeze(1)
        old = Xn[:, k, :]
        upd = torch.clamp(old + (Na[:, k, :] - l1_den - gx - l2 * old) / diag, min=0.0)
        Xn[:, k, :] = torch.where(diag > eps, upd, old)
    return Xn


def solve(algo: int, x, numer, gram, rep_index, max_iter, tol, l1_num, l1_den, l2, eps,
          lin_out, quad_out, iters_out, nsplit=1, conv_mode=0, check_every=10,
          active=None) -> None:
    R, K, n = x.shape
    reps = (torch.arange(R, device=x.device) if rep_index is None
            else rep_index.to(device=x.device, dtype=torch.long))
    if active is not None:
        reps = reps[active.to(x.device)[reps] != 0]
    if reps.numel() == 0:
        return
    X = x[reps].clone()
    N = numer[reps].to(X.dtype)
    if l1_num > 0:
        N = torch.clamp(N - l1_num, min=0.0)
    G = gram[reps].to(X.dtype)
    m = reps.numel()
    active = torch.ones(m, dtype=torch.bool, device=x.device)
    iters = torch.zeros(m, dtype=torch.int32, device=x.device)
    check = nsplit <= 1
    loss_conv = check and conv_mode == 1
    every = max(1, int(check_every))
    f_prev = torch.zeros(m, dtype=X.dtype, device=x.device)
    have_prev = False
    it = 0
    while True:
        if loss_conv and it % every == 0:
            idx = torch.nonzero(active).flatten()
            if idx.numel() == 0:
                break
            f = _objective(X[idx], N[idx], G[idx], l1_den, l2)
            if have_prev:
                conv = torch.abs(f_prev[idx] - f) <= tol * torch.abs(f_prev[idx])
                active[idx[conv]] = False
            f_prev[idx] = f
            have_prev = True
        if it >= int(max_iter):
            break
        idx = torch.nonzero(active).flatten()
        if idx.numel() == 0:
            break
        Xa = X[idx]
        Xn = _step(algo, Xa, N[idx], G[idx], l1_den, l2, eps)
        X[idx] = Xn
        iters[idx] += 1
        it += 1
        if check and not loss_conv:
            d2 = ((Xn - Xa) ** 2).sum(dim=(1, 2))
            x2 = (Xa ** 2).sum(dim=(1, 2))
            conv = torch.sqrt(d2) / (torch.sqrt(x2) + eps) < tol
            active[idx[conv]] = False
    x[reps] = X
    if lin_out is not None or quad_out is not None:
        lin = (numer[reps].to(X.dtype) * X).sum(dim=(1, 2))
        quad = (X * torch.bmm(G, X)).sum(dim=(1, 2))
        if lin_out is not None:
            lin_out[reps] = lin.to(lin_out.dtype)
        if quad_out is not None:
            quad_out[reps] = quad.to(quad_out.dtype)
    if iters_out is not None:
        iters_out[reps] += iters.to(iters_out.dtype)


def philox_fill(out: torch.Tensor, seeds, scales, stream: int, mode: int = 0,
                row_offset: int = 0) -> None:
    R, rows, cols = out.shape
    seeds = [int(s) for s in torch.as_tensor(seeds).cpu().tolist()]
    scales = torch.as_tensor(scales, dtype=torch.float32).cpu()
    for r in range(R):
        m = torch.from_numpy(philox_matrix(seeds[r], stream, rows, cols, mode, row_offset))
        out[r].copy_((m * scales[r]).to(out.dtype))


def _sqrt_f64(x: torch.Tensor) -> torch.Tensor:
    """Correctly rounded square root, as the device's: torch's vectorised CPU sqrt is
    1 ulp off for some float64 inputs, numpy's is the IEEE one."""
    if x.device.type != "cpu":
        return torch.sqrt(x)
    with np.errstate(invalid="ignore"):
        return torch.from_numpy(np.sqrt(x.contiguous().numpy()))


def conv_update(lin, quad, x_sq, state, n, pass_idx, tol, final, init=False, max_pass=0):
    # (clamp keeps a NaN radicand NaN: non-finite statistics propagate, as in conv.hip)
    e = _sqrt_f64(torch.clamp(x_sq - 2.0 * lin[:n].double() + quad[:n].double(), min=0.0))
    e = e.to(state["err"].device)
    if init:
        for k in ("err_init", "err_prev", "err"):
            state[k][:n] = e
        state["active"][:n] = 1
        state["converged"][:n] = 0
        state["n_pass"][:n] = 0
        return
    act = state["active"][:n] != 0
    state["err"][:n] = torch.where(act, e, state["err"][:n])
    new_pass = (torch.full_like(state["n_pass"][:n], pass_idx) if pass_idx >= 0
                else state["n_pass"][:n] + 1)              # pass_idx < 0: count passes
    state["n_pass"][:n] = torch.where(act, new_pass, state["n_pass"][:n])
    rel = (state["err_prev"][:n] - e) / torch.clamp(state["err_init"][:n], min=1e-300)
    conv = act & (rel < tol)
    over = (new_pass >= max_pass) if max_pass > 0 else torch.zeros_like(act)
    stop = conv | (act & (bool(final) | over))
    state["converged"][:n] = torch.where(conv, torch.ones_like(state["converged"][:n]),
                                         state["converged"][:n])
    keep = act & ~stop
    state["err_prev"][:n] = torch.where(keep, e, state["err_prev"][:n])
    state["active"][:n] = torch.where(stop, torch.zeros_like(state["active"][:n]),
                                      state["active"][:n])


def beta_terms(X: torch.Tensor, P: torch.Tensor, beta: float, eps: float):
    """Q = X * P^(beta-2), D = P^(beta-1) with P clamped at eps (beta_mu.hip)."""
    Pc = torch.clamp(P, min=eps)
    if beta == 1.0:
        return X / Pc, None
    if beta == 0.0:
        r = Pc.reciprocal()
        return X * r * r, r
    return X * Pc ** (beta - 2.0), Pc ** (beta - 1.0)


def beta_loss_terms(X: torch.Tensor, P: torch.Tensor, beta: float, eps: float) -> torch.Tensor:
    Pc = torch.clamp(P, min=eps)
    if beta == 1.0:
        pos = X > 0
        t = torch.where(pos, X * torch.log(torch.where(pos, X, torch.ones_like(X)) / Pc),
                        torch.zeros_like(Pc))
        return t - X + Pc
    if beta == 0.0:
        d = torch.clamp(X / Pc, min=eps)
        return d - torch.log(d) - 1.0
    return (X ** beta + (beta - 1.0) * Pc ** beta - beta * X * Pc ** (beta - 1.0)) / (
        beta * (beta - 1.0))


def beta_contract(side: int, X, HT3, W3, beta: float, eps: float, want_num: bool = True,
                  want_loss: bool = False, active=None, row_chunk: int = 4096):
    """Reference of cnmf_beta_contract: returns (num, den, loss) with num/den (R,K,N) for
    side 0 (H) and (R,K,G) for side 1 (W); den is None for beta == 1; loss (R,) float64
    (side 0 only) or None.  Inactive replicates get zeros."""
    R, K, N = HT3.shape
    G = W3.shape[2]
    dt = HT3.dtype
    out_n = N if side == 0 else G
    num = torch.zeros((R, K, out_n), dtype=dt, device=HT3.device) if want_num else None
    den = (torch.zeros((R, K, out_n), dtype=dt, device=HT3.device)
           if (want_num and beta != 1.0) else None)
    loss = torch.zeros(R, dtype=torch.float64, device=HT3.device) if (want_loss and side == 0) else None
    reps = range(R) if active is None else [r for r in range(R) if int(active[r]) != 0]
    for r in reps:
        for a in range(0, N, row_chunk):
            b = min(N, a + row_chunk)
            x = X[a:b].to(dt)
            h = HT3[r, :, a:b]                      # (K, c)
            P = h.t() @ W3[r]                       # (c, G)
            Q, D = beta_terms(x, P, beta, eps)
            if want_num:
                if side == 0:
                    num[r, :, a:b] = W3[r] @ Q.t()
                    if D is not None:
                        den[r, :, a:b] = W3[r] @ D.t()
                else:
                    num[r] += h @ Q
                    if D is not None:
                        den[r] += h @ D
            if loss is not None:
                loss[r] += beta_loss_terms(x.double(), P.double(), beta, eps).sum()
    return num, den, loss


def beta_update_h(X, HT3, W3, beta, eps, l1=0.0, l2=0.0, gamma=1.0, act=None, tol=None,
                  iters=None, conv_mode=0, check_every=10, hstate=None, contract=None):
    """Reference of the fused in-place usage update (beta_mu.hip, upd != 0).  ``contract``:
    the beta_contract implementation to use (ops: the rank-general native one)."""
    beta_contract_ = contract or beta_contract
    R = HT3.shape[0]
    loss_rule = tol is not None and conv_mode == 1
    num, den, f = beta_contract_(0, X, HT3, W3, beta, eps, True, loss_rule, act)
    if den is None:
        den = W3.sum(dim=2, keepdim=True)
    d = den + l1 + l2 * HT3
    d = torch.where(d == 0, torch.full_like(d, eps), d)
    delta = num / d
    if gamma != 1.0:
        delta = delta ** gamma
    live = torch.ones(R, dtype=torch.bool, device=HT3.device) if act is None else (act[:R] != 0)
    delta = torch.where(live.view(R, 1, 1), delta, torch.ones_like(delta))
    if tol is not None and not loss_rule:
        dn = torch.linalg.vector_norm((HT3 * (delta - 1.0)).double(), dim=(1, 2))
        hn = torch.linalg.vector_norm(HT3.double(), dim=(1, 2))
    HT3.mul_(delta)
    if tol is not None:
        if loss_rule:
            hs = hstate.view(-1, 2)[:R]
            f = f.to(hs.device)
            steps = hs[:, 1].long()
            every = max(1, int(check_every))
            at_check = live & (steps % every == 0)
            conv = at_check & (steps > 0) & ((hs[:, 0] - f).abs() <= tol * hs[:, 0].abs())
            hs[:, 0] = torch.where(at_check, f, hs[:, 0])
            hs[:, 1] = torch.where(live, hs[:, 1] + 1, hs[:, 1])
            stop = conv
        else:
            stop = live & (dn / (hn + eps) < tol)
        act[:R][stop] = 0
        if iters is not None:
            iters[:R] += live.to(iters.dtype)


def beta_h_block(X, HT3, W3, beta, eps, nsteps, l1=0.0, l2=0.0, gamma=1.0, act=None, tol=None,
                 iters=None, conv_mode=1, hstate=None, loss_entry=False, contract=None):
    """Reference of the multi-step usage solve block (beta_planes.hip, side 0): ``nsteps``
    MU steps of the live replicates, then the stopping rule: conv_mode 1 compares the
    block's exit objective -- the beta-divergence at the iterate its last step starts from
    (after the block for a one-step block) -- with the previous one (``loss_entry``: the
    objective before the block, evaluated here; else the value ``hstate`` recorded);
    conv_mode 0 reads the relative change of the block's last step."""
    beta_contract_ = contract or beta_contract
    R = HT3.shape[0]
    live = torch.ones(R, dtype=torch.bool, device=HT3.device) if act is None else (act[:R] != 0)
    rule = tol is not None
    f_entry = None
    if rule and conv_mode == 1 and loss_entry and nsteps > 0:
        f_entry = beta_contract_(0, X, HT3, W3, beta, eps, False, True, act)[2].to(HT3.device)
    dn = hn = None
    f_exit = None
    exit_in_last = nsteps >= 2
    for s in range(nsteps):
        # the kernel reads the exit objective off the last step's P pass (here: the same
        # contraction returns it)
        at_exit = rule and conv_mode == 1 and exit_in_last and s == nsteps - 1
        num, den, f = beta_contract_(0, X, HT3, W3, beta, eps, True, at_exit, act)
        if at_exit:
            f_exit = f.to(HT3.device)
        if den is None:
            den = W3.sum(dim=2, keepdim=True)
        d = den + l1 + l2 * HT3
        d = torch.where(d == 0, torch.full_like(d, eps), d)
        delta = num / d
        if gamma != 1.0:
            delta = delta ** gamma
        delta = torch.where(live.view(R, 1, 1), delta, torch.ones_like(delta))
        if s == nsteps - 1 and rule and conv_mode == 0:
            dn = torch.linalg.vector_norm((HT3 * (delta - 1.0)).double(), dim=(1, 2))
            hn = torch.linalg.vector_norm(HT3.double(), dim=(1, 2))
        HT3.mul_(delta)
    if not rule:
        return
    if conv_mode == 1:
        if f_exit is None:
            f_exit = beta_contract_(0, X, HT3, W3, beta, eps, False, True, act)[2].to(HT3.device)
        hs = hstate.view(-1, 2)[:R]
        f_prev = f_entry if loss_entry else hs[:, 0]
        checked = torch.full_like(live, bool(loss_entry)) | (hs[:, 1] > 0)
        stop = live & checked & ((f_prev - f_exit).abs() <= tol * f_prev.abs())
        hs[:, 0] = torch.where(live, f_exit, hs[:, 0])
        hs[:, 1] = torch.where(live, hs[:, 1] + 1, hs[:, 1])
    elif nsteps > 0:
        stop = live & (dn / (hn + eps) < tol)
    else:
        stop = torch.zeros_like(live)
    act[:R][stop] = 0
    if iters is not None:
        iters[:R] += live.to(iters.dtype) * int(nsteps)


def beta_w_update(W3, num, den, hsum, An, Ad, an_out, dn_out, beta, gamma, l1, l2, eps, tol,
                  act, iters=None):
    """Reference of the anchored online spectra step (beta_mu.hip beta_w_update_kernel)."""
    R = W3.shape[0]
    live = act[:R] != 0
    if not bool(live.any()):
        return
    nu = num.sum(0)
    kl = beta == 1.0
    dn = hsum.unsqueeze(2).expand_as(nu) if kl else den.sum(0)
    ad = Ad.unsqueeze(2) if kl else Ad
    an = W3 ** (1.0 / gamma) * nu
    B = ad + dn + l1 + l2 * W3
    B = torch.where(B == 0, torch.full_like(B, eps), B)
    Wn = ((An + an) / B) ** gamma
    m = live.view(R, 1, 1)
    d = torch.linalg.vector_norm(torch.where(m, Wn - W3, 0).double(), dim=(1, 2))
    o = torch.linalg.vector_norm(W3.double(), dim=(1, 2))
    W3.copy_(torch.where(m, Wn, W3))
    an_out.copy_(torch.where(m, an, an_out))
    if not kl:
        dn_out.copy_(torch.where(m, dn, dn_out))
    stop = live & (d / (o + eps) < tol)
    act[:R][stop] = 0
    if iters is not None:
        iters[:R] += live.to(iters.dtype)


def _bf16_rn_bits(v: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even bf16 bit patterns (int32 holding 16 bits) of finite fp32."""
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u & 0xFFFF).to(torch.int32)


def _bits_to_f32(h: torch.Tensor) -> torch.Tensor:
    return (h.to(torch.int64) << 16).to(torch.int32).view(torch.float32)


def split_planes(S: torch.Tensor, nplanes: int, ld: int) -> torch.Tensor:
    """(nplanes, rows, ld) int16 bf16 planes of fp32 S (columns beyond S are zero)."""
    rows, cols = S.shape
    out = torch.zeros((nplanes, rows, ld), dtype=torch.int16, device=S.device)
    r = S.to(torch.float32)
    for p in range(nplanes):
        h = _bf16_rn_bits(r)
        out[p, :, :cols] = h.to(torch.int16)   # wraps to the same 16-bit pattern
        r = r - _bits_to_f32(h)
    return out


def planes_to_f64(P: torch.Tensor) -> torch.Tensor:
    """bf16 planes (P, rows, k) int16 -> their float64 values, per plane."""
    return _bits_to_f32(P.to(torch.int32) & 0xFFFF).to(torch.float64)


def gemm_planes(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """sum_{i + j <= 2} A_i B_j^T in float64 (oracle of ops.gemm_planes)."""
    Af, Bf = planes_to_f64(A), planes_to_f64(B)
    out = torch.zeros((A.shape[1], B.shape[1]), dtype=torch.float64, device=A.device)
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            if i + j <= 2:
                out += Af[i] @ Bf[j].t()
    return out


def tiles_to_planes(tiles, r0: int = 0, r1: int | None = None) -> torch.Tensor:
    """(pb, r1 - r0, G) int16 bf16 planes of rows [r0, r1) of an ops.XTiles matrix."""
    r1 = tiles.N if r1 is None else r1
    ntg = -(-tiles.G // 64)
    t0, t1 = r0 // 64, -(-r1 // 64)                    # row tiles the range touches
    ptr = tiles.ptr[t0 * ntg:t1 * ntg + 1]
    e0, e1 = (int(ptr[0]), int(ptr[-1])) if r1 > r0 else (0, 0)
    ent = tiles.ent[e0:e1].to(torch.int64) & 0xFFFFFFFF
    tid = torch.repeat_interleave(torch.arange(t0 * ntg, t1 * ntg, device=ent.device),
                                  torch.diff(ptr)) if e1 > e0 else ent
    row = torch.div(tid, ntg, rounding_mode="floor") * 64 + ((ent >> 22) & 63)
    col = (tid % ntg) * 64 + ((ent >> 16) & 63)
    keep = (row >= r0) & (row < r1)
    out = torch.zeros((tiles.pb, r1 - r0, tiles.G), dtype=torch.int16, device=ent.device)
    vals = [(ent & 0xFFFF).to(torch.int32)] + [x[e0:e1].to(torch.int32) & 0xFFFF
                                               for x in tiles.extra]
    for p, v in enumerate(vals):
        v16 = torch.where(v >= 32768, v - 65536, v).to(torch.int16)
        out[p].index_put_((row[keep] - r0, col[keep]), v16[keep])
    return out


def gemm_tiles(A: torch.Tensor, tiles, side: str, r0: int, r1: int) -> torch.Tensor:
    """Oracle of ops.gemm_tiles in float64: the tiles' rows [r0, r1) densified, then the
    plane-pair sum of gemm_planes.  A: (pa, M, k) int16 planes."""
    Xf = planes_to_f64(tiles_to_planes(tiles, r0, r1))          # (pb, rows, G)
    Af = planes_to_f64(A)
    n = r1 - r0
    out = torch.zeros((A.shape[1], n if side == "n" else tiles.G), dtype=torch.float64,
                      device=A.device)
    for i in range(A.shape[0]):
        for j in range(Xf.shape[0]):
            if i + j <= 2:
                out += Af[i][:, :tiles.G] @ Xf[j].t() if side == "n" else Af[i][:, :n] @ Xf[j]
    return out


def colstats(X: torch.Tensor):
    inf = torch.tensor(float("inf"), dtype=X.dtype, device=X.device)
    mn = torch.where(X > 0, X, inf).amin(0) if X.shape[0] else \
        torch.full((X.shape[1],), float("inf"), dtype=X.dtype, device=X.device)
    sq = (X.to(torch.float64) ** 2).sum(0)
    neg = (X < 0).any(0).to(torch.int32)
    return mn, sq, neg


def count_unit_check(X: torch.Tensor, mn: torch.Tensor) -> torch.Tensor:
    bad = torch.zeros(X.shape[1], dtype=torch.int32, device=X.device)
    ok_col = (mn > 0) & torch.isfinite(mn)
    for d in range(1, 9):
        c = X / (mn / d)
        off = ((c - torch.round(c)).abs() > 4e-7 * c + 1e-4) | (c >= 65535.5)
        off &= X != 0
        bad |= (off.any(0) & ok_col).to(torch.int32) << (d - 1)
    return bad


def csr_transpose_tiles(rowptr, col, val, a: int, b: int, G: int, tl: int) -> list:
    """Transposed tile CSRs of rows [a, b) of a CSR matrix (``rowptr`` with absolute
    offsets, ``col``, ``val``; torch tensors or numpy arrays) -- the contract of
    csr_transpose.hip: [(t0, rowptr_t (G + 1, int32, from 0), col_t (int32), val_t
    (float32))] over tiles of ``tl`` rows, tile t the CSR of X[a + t0 : a + t1]^T with G
    rows, the cell's index inside the tile as column, ascending within a gene."""
    rp = torch.as_tensor(rowptr).to(torch.int64).cpu()
    col = torch.as_tensor(col).cpu()
    val = torch.as_tensor(val).cpu()
    out = []
    for t0 in range(0, b - a, tl):
        t1 = min(b - a, t0 + tl)
        lo, hi = int(rp[a + t0]), int(rp[a + t1])
        g = col[lo:hi].to(torch.int64)
        cell = torch.repeat_interleave(torch.arange(t1 - t0), torch.diff(rp[a + t0:a + t1 + 1]))
        order = torch.argsort(g * (t1 - t0) + cell)       # (gene, cell) keys are unique
        rpt = torch.zeros(G + 1, dtype=torch.int64)
        rpt[1:] = torch.bincount(g, minlength=G).cumsum(0)
        out.append((t0, rpt.to(torch.int32), cell[order].to(torch.int32),
                    val[lo:hi].to(torch.float32)[order]))
    return out



def csr_transpose(rowptr, col, val, n: int, G: int):
    """Torch twin of ops.csr_transpose: (rowptr (G + 1, int32, from 0), col (int32, the
    source row), val) of the transpose of an (n x G) CSR, the entries of a transposed row
    ordered by source row (a stable sort by column of the row-major entries)."""
    rp = rowptr.long()
    lo, hi = (int(rp[0]), int(rp[n])) if n else (0, 0)
    c = col[lo:hi].long()
    rows = torch.repeat_interleave(torch.arange(n, device=c.device), rp[1:n + 1] - rp[:n])
    order = torch.sort(c, stable=True).indices
    out_rp = torch.zeros(G + 1, dtype=torch.int64, device=c.device)
    if hi > lo:
        out_rp[1:] = torch.bincount(c, minlength=G).cumsum(0)
    pad = 1 if hi == lo else 0      # the kernels' clamped loads read entry 0
    out_col = torch.zeros(hi - lo + pad, dtype=torch.int32, device=c.device)
    out_val = torch.zeros(hi - lo + pad, dtype=val.dtype, device=c.device)
    out_col[:hi - lo] = rows[order].to(torch.int32)
    out_val[:hi - lo] = val[lo:hi][order]
    return out_rp.to(torch.int32), out_col, out_val


def kl_refit(csr, HT, W, chunk_size, max_iter, tol, l1=0.0, l2=0.0, eps=1e-16, iters=None,
             trace=None):
    """Reference of ops.kl_sparse_refit (sparse_kl.hip, chunk-batched usage step), in the
    dtype of HT: for every chunk of ``chunk_size`` rows of the CSR matrix ``csr`` (rowptr,
    col, val, n, G), up to ``max_iter`` KL MU steps of HT[:, chunk] (K x c) against the
    fixed W (K x G) -- p = eps + h . W[:, g] on the stored entries, num = sum_g W_kg x / p,
    denominator sum_g W_kg + l1 + l2 h (eps where it is 0) -- until the step's iterate change
    ||h_new - h|| / (||h|| + eps) < tol.  ``iters``: per-chunk step counts are added.
    ``trace``: a list that receives (chunk, step, change) of every step."""
    rowptr, col, val, n, G = csr
    K = HT.shape[0]
    dt = HT.dtype
    Wd = W.to(dt)
    WT = Wd.t().contiguous()
    den0 = Wd.sum(dim=1)
    c = max(1, min(int(chunk_size), int(n))) if n else 1
    rp = rowptr.long()
    for ci, a in enumerate(range(0, n, c)):
        b = min(n, a + c)
        lo, hi = int(rp[a]), int(rp[b])
        S = WT[col[lo:hi].long()]                                # (e, K)
        x = val[lo:hi].to(dt)
        rows = torch.repeat_interleave(torch.arange(b - a, device=HT.device),
                                       rp[a + 1:b + 1] - rp[a:b])
        h = HT[:, a:b].clone()
        steps = 0
        for _ in range(int(max_iter)):
            p = eps + (S * h.t()[rows]).sum(dim=1)
            q = x / p
            num = torch.zeros((b - a, K), dtype=dt, device=HT.device)
            num.index_add_(0, rows, q[:, None] * S)
            dn = den0[:, None] + l1 + l2 * h
            dn = torch.where(dn == 0, torch.full_like(dn, eps), dn)
            hn = h * (num.t() / dn)
            rel = float(torch.linalg.vector_norm((hn - h).double())
                        / (torch.linalg.vector_norm(h.double()) + eps))
            h = hn
            steps += 1
            if trace is not None:
                trace.append((ci, steps, rel))
            if rel < tol:
                break
        HT[:, a:b] = h
        if iters is not None:
            iters[ci] += steps


# ---------------------------------------------------------------------------------------
# Mutual information of continuous features against a discrete target (Ross 2014), as
# scikit-learn 1.7's mutual_info_classif computes it on a dense matrix
# (docs/ARCHITECTURE.md "Mutual information").  CPU implementation and oracle of mi_cd.hip.

MI_MAX_NEIGHBORS = 8


def _mi_rng(random_state):
    """sklearn's check_random_state: None -> numpy's global RandomState, an int -> a fresh
    RandomState, a RandomState -> itself."""
    if random_state is None or random_state is np.random:
        return np.random.mtrand._rand
    if isinstance(random_state, np.random.RandomState):
        return random_state
    return np.random.RandomState(int(random_state))


def mi_prepare(X, random_state=None, row_block: int = 4096) -> np.ndarray:
    """The float64 matrix scikit-learn's ``_estimate_mi`` hands to its per-feature
    estimator, bit for bit: every column divided by its ``nanstd`` (1 where that is below
    10 eps), then ``1e-10 * max(1, mean|x|) * N(0, 1)`` noise added.  The noise is drawn
    row-major in blocks of ``row_block`` rows, which is the same RandomState stream as one
    draw of the whole matrix, without a second (n, G) array.

    The result is column-major.  scikit-learn takes the two column statistics on
    ``X[:, mask]``, which numpy returns column-major, so every column is reduced pairwise
    over contiguous memory; the same reductions of a row-major matrix differ in the last
    bit, which moves a neighbour count wherever a squared distance sits on its radius."""
    X = np.array(X, dtype=np.float64, order="F")        # a copy, like copy=True
    if X.ndim != 2:
        raise ValueError("mi_prepare: a 2-D matrix is required")
    n, G = X.shape
    std = np.nanstd(X, axis=0)
    std[std < 10 * np.finfo(np.float64).eps] = 1.0
    X /= std
    scale = 1e-10 * np.maximum(1, np.mean(np.abs(X), axis=0))
    rng = _mi_rng(random_state)
    step = max(1, int(row_block))
    for a in range(0, n, step):
        b = min(n, a + step)
        X[a:b] += scale * rng.standard_normal(size=(b - a, G))
    return X


def mi_class_terms(codes, n_neighbors: int):
    """The feature-independent part of the estimator for integer class ``codes`` (n,):
    (keep, counts, const) with ``keep`` the mask of points whose class has >= 2 members,
    ``counts`` the class size of every kept point and
    ``const = psi(n') + mean psi(k_i) - mean psi(N_i)``, k_i = min(n_neighbors, N_i - 1)."""
    from scipy.special import digamma

    codes = np.asarray(codes)
    _, inv, cnt = np.unique(codes, return_inverse=True, return_counts=True)
    size = cnt[inv.reshape(-1)]
    keep = size > 1
    counts = size[keep]
    n_kept = int(keep.sum())
    if n_kept == 0:
        return keep, counts, 0.0
    k_all = np.minimum(int(n_neighbors), counts - 1)
    const = (digamma(n_kept) + np.mean(digamma(k_all.astype(np.float64)))
             - np.mean(digamma(counts.astype(np.float64))))
    return keep, counts, float(const)


def mi_psi_table(n: int) -> np.ndarray:
    """digamma(1..n) in float64 (entry m - 1 is psi(m)): what both backends add."""
    from scipy.special import digamma

    return digamma(np.arange(1, int(n) + 1, dtype=np.float64))


def _mi_reach(v, g, rad2, right: bool):
    """Per point the last (right) / first (left) sorted index j, outward from its own rank
    g, with fl((v[j] - v[g])^2) <= rad2: a vectorised bisection (the predicate holds at g
    and is monotone outward)."""
    n = v.shape[0]
    ok = g.copy()
    bad = np.full(n, n if right else -1, dtype=np.int64)
    vg = v[g]
    while True:
        open_ = np.abs(bad - ok) > 1
        if not open_.any():
            return ok
        mid = (ok + bad) // 2
        d = v[np.clip(mid, 0, n - 1)] - vg
        hold = open_ & (d * d <= rad2)
        ok = np.where(hold, mid, ok)
        bad = np.where(open_ & ~hold, mid, bad)


def mi_cd(Xp, codes, n_neighbors: int = 3):
    """(mi (G,) float64, m (n, G) int32) of the prepared float64 matrix ``Xp`` (n, G)
    against the integer class ``codes`` (n,).  Points whose class occurs once are dropped
    (m = 0 there).  For a kept point i of a class of N_i points: k_i = min(n_neighbors,
    N_i - 1), r_i = the distance |c_j - c_i| to its k_i-th nearest neighbour of the class,
    radius_i = nextafter(r_i, 0), and m_i counts the kept points j of every class, i
    included, with fl((c_j - c_i)^2) <= fl(radius_i^2).  mi = psi(n') + mean psi(k_i) -
    mean psi(N_i) - mean psi(m_i), before the clamp at 0 that the caller applies
    (models.mi).  Distances are exact differences for every class size; scikit-learn's
    brute-force neighbour search for classes of 3 to 7 points is not imitated."""
    Xp = np.asarray(Xp)
    if Xp.dtype != np.float64 or Xp.ndim != 2:
        raise ValueError("mi_cd: a 2-D float64 matrix is required")
    nn = int(n_neighbors)
    if not 1 <= nn <= MI_MAX_NEIGHBORS:
        raise ValueError(f"mi_cd: n_neighbors must be in 1..{MI_MAX_NEIGHBORS}")
    if not np.isfinite(Xp).all():
        raise ValueError("mi_cd: non-finite input")
    n, G = Xp.shape
    codes = np.asarray(codes).reshape(-1)
    if codes.shape[0] != n:
        raise ValueError("mi_cd: one code per row is required")
    keep, counts, const = mi_class_terms(codes, nn)
    mi = np.zeros(G, dtype=np.float64)
    m_all = np.zeros((n, G), dtype=np.int32)
    n_kept = int(keep.sum())
    if n_kept == 0:
        return mi, m_all
    rows = np.flatnonzero(keep)
    ck = codes[keep]
    k_all = np.minimum(nn, counts - 1)
    pos = np.arange(n_kept)
    psi = mi_psi_table(n_kept)
    for f in range(G):
        c = Xp[keep, f]
        order = np.argsort(c, kind="stable")
        v = c[order]
        cls = ck[order]
        ranks = np.argsort(cls, kind="stable")          # class order -> sorted position
        cs = cls[ranks]
        start = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
        a = np.repeat(start, np.diff(np.r_[start, n_kept]))     # segment bounds per slot
        b = np.repeat(np.r_[start[1:], n_kept], np.diff(np.r_[start, n_kept]))
        vq = v[ranks]
        D = np.full((n_kept, 2 * nn), np.inf)
        for j in range(1, nn + 1):
            left = pos - j >= a
            D[left, 2 * j - 2] = vq[left] - vq[pos[left] - j]
            right = pos + j < b
            D[right, 2 * j - 1] = vq[pos[right] + j] - vq[right]
        D.sort(axis=1)
        r = D[pos, k_all[order][ranks] - 1]
        radius = np.nextafter(r, 0.0)
        rad2 = radius * radius
        hi = _mi_reach(v, ranks, rad2, True)
        lo = _mi_reach(v, ranks, rad2, False)
        m_all[rows[order[ranks]], f] = (hi - lo + 1).astype(np.int32)
        mi[f] = const - np.mean(psi[m_all[rows, f] - 1])    # mean in row order, as sklearn
    return mi, m_all


# ---------------------------------------------------------------------------------------
# LOESS: local polynomial regression with tricube weights over the k nearest points, the
# direct fit of models/pp.py ``loess_fit`` in O(block * k) memory (docs/ARCHITECTURE.md
# "LOESS").  CPU implementation and oracle of loess.hip.

LOESS_BLOCK = 256
LOESS_RIDGE = 1e-10
LOESS_H_FACTOR = 1.0000001


def loess_k(n: int, span: float, degree: int) -> int:
    """Window size of a series of n points: min(n, max(degree + 1, ceil(span * n)))."""
    return int(min(n, max(degree + 1, int(np.ceil(span * n)))))


def loess_offsets(offsets, n: int) -> np.ndarray:
    """``offsets`` as a validated int64 array of B + 1 series bounds over n points (None: one
    series): starts at 0, never decreases, ends at n."""
    if offsets is None:
        return np.array([0, int(n)], dtype=np.int64)
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.cpu().numpy()
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 2 or off.dtype.kind not in "iu":
        raise ValueError("loess: offsets must be a 1-D integer array of B + 1 bounds")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != int(n) or (np.diff(off) < 0).any():
        raise ValueError("loess: offsets must start at 0, never decrease and end at len(x)")
    return off


def loess_windows(xs, k: int) -> np.ndarray:
    """Window starts (int64) of the sorted float64 series ``xs`` for windows of k points:
    start_i is the first lo in [0, n - k] at which ``xs[lo + k] - xs[i] < xs[i] - xs[lo]`` is
    false (lo = n - k counts as false).  The predicate is monotone in lo, so a bisection per
    point, with no state carried between points, finds it; its first-false point does not
    decrease with i, so this is where the sliding loop of ``pp.loess_fit`` stops."""
    xs = np.asarray(xs, dtype=np.float64)
    n, k = xs.shape[0], int(k)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    if not 1 <= k <= n:
        raise ValueError("loess_windows: k must be in 1..len(xs)")
    lo = np.zeros(n, dtype=np.int64)
    hi = np.full(n, n - k, dtype=np.int64)
    while True:
        open_ = lo < hi
        if not open_.any():
            return lo
        mid = (lo + hi) // 2                         # < n - k wherever open
        step = open_ & ((xs[np.minimum(mid + k, n - 1)] - xs) < (xs - xs[mid]))
        lo = np.where(step, mid + 1, lo)
        hi = np.where(open_ & ~step, mid, hi)


def _loess_solve0(S, T):
    """First component of (S_{a+b} + ridge I)^-1 T for every row: Gaussian elimination with
    partial pivoting (the first row of the largest magnitude), elementwise over the rows."""
    m = len(T)
    A = np.empty((S[0].shape[0], m, m + 1), dtype=np.float64)
    for a in range(m):
        for c in range(m):
            A[:, a, c] = S[a + c] + (LOESS_RIDGE if a == c else 0.0)
        A[:, a, m] = T[a]
    for c in range(m):
        for r in range(c + 1, m):
            swap = np.abs(A[:, r, c]) > np.abs(A[:, c, c])
            A[swap, c], A[swap, r] = A[swap, r], A[swap, c]
        for r in range(c + 1, m):
            f = A[:, r, c] / A[:, c, c]
            A[:, r, c:] -= f[:, None] * A[:, c, c:]
    coef = [None] * m
    for a in range(m - 1, -1, -1):
        v = A[:, a, m].copy()
        for c in range(a + 1, m):
            v -= A[:, a, c] * coef[c]
        coef[a] = v / A[:, a, a]
    return coef[0]


def _loess_sorted(xs, ys, k: int, starts, degree: int, block: int, points=None) -> np.ndarray:
    """Fitted values of the sorted series at its own points (or at the sorted positions
    ``points`` only), ``block`` points at a time."""
    pts = np.arange(xs.shape[0]) if points is None else np.asarray(points, dtype=np.int64)
    out = np.empty(pts.shape[0], dtype=np.float64)
    win = np.arange(k)
    for a in range(0, pts.shape[0], block):
        i = pts[a:a + block]
        s = starts[i]
        idx = s[:, None] + win[None, :]
        xi = xs[i]
        d = xs[idx] - xi[:, None]
        yw = ys[idx]
        h = np.maximum(xi - xs[s], xs[s + k - 1] - xi)      # = |d|.max(): the window is sorted
        h = np.where(h > 0, h * LOESS_H_FACTOR, 1.0)
        r = np.abs(d) / h[:, None]
        u = np.maximum(1.0 - r * r * r, 0.0)
        pw = u * u * u                                       # w d^p
        S, T = [], []
        for p in range(2 * degree + 1):
            S.append(pw.sum(axis=1))
            if p <= degree:
                T.append((pw * yw).sum(axis=1))
            pw = pw * d
        out[a:a + i.shape[0]] = _loess_solve0(S, T)
    return out


def loess(x, y, offsets=None, span: float = 0.3, degree: int = 2, block: int = LOESS_BLOCK,
          return_windows: bool = False):
    """Fitted values (float64, input order) of the local regression of y on x at the points
    themselves, for B independent series laid end to end: series b is
    ``[offsets[b], offsets[b + 1])`` (ragged, possibly empty; None: one series).

    Per series of n points: stable sort by x, k = ``loess_k(n, span, degree)``, window starts
    by :func:`loess_windows`.  Per point i with d = x_window - x_i: h = the larger distance to
    the two window ends, times 1.0000001, or 1 when it is 0; w = max(1 - (|d| / h)^3, 0)^3;
    S_p = sum w d^p (p <= 2 degree), T_p = sum w d^p y (p <= degree), the powers formed by
    multiplication; the fitted value is the first component of (S_{a+b} + 1e-10 I)^-1 T by
    Gaussian elimination with partial pivoting.  ``block`` points are in flight at a time
    (memory O(block * k)); every row is reduced on its own, so the result does not depend on
    ``block``.  ``return_windows``: also the window starts (int64, inside each series, sorted
    order) and the sort order (int64 indices into x, series by series)."""
    degree = int(degree)
    if degree not in (1, 2):
        raise ValueError("loess: degree must be 1 or 2")
    if not float(span) > 0:
        raise ValueError("loess: span must be positive")
    if int(block) < 1:
        raise ValueError("loess: block must be positive")
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError("loess: x and y must have the same length")
    off = loess_offsets(offsets, x.shape[0])
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("loess: non-finite input")
    fitted = np.empty(x.shape[0], dtype=np.float64)
    starts_all = np.zeros(x.shape[0], dtype=np.int64)
    order_all = np.zeros(x.shape[0], dtype=np.int64)
    for a, b in zip(off[:-1], off[1:]):
        if b == a:
            continue
        order = np.argsort(x[a:b], kind="stable")
        xs, ys = x[a:b][order], y[a:b][order]
        k = loess_k(b - a, span, degree)
        starts = loess_windows(xs, k)
        fit = _loess_sorted(xs, ys, k, starts, degree, int(block))
        fitted[a + order] = fit
        starts_all[a:b] = starts
        order_all[a:b] = a + order
    return (fitted, starts_all, order_all) if return_windows else fitted
