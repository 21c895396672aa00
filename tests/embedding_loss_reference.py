"""Float64 reference of the pixel-embedding loss on the device (pctrans_amd/embedding_loss.py; kernels csrc/embedding_loss.hip),
the label map's restatement, and the bound the tests hold the fp32 results to.  Nothing here depends on the code under test.

`loss64` restates the reference's per-instance loop (loss/loss.py:297-355) in float64 and differentiates it with autograd.

Bound (`bounds`), from the kernels' arithmetic, u = 2^-24, per image; n_g pixels of label g, `chunks` from the header's split:

* centroid.  A channel sum is an fmaf chain over the label's n_g pixels inside the chunks (the products with the 0 / 1 operand are
  exact), `chunks` additions join them, one division: channel c of mu_g is within (n_g + chunks + 1) u mean_p |e_p[c]|; e_mu(g) is
  the Euclidean norm of that over the channels.
* per pixel.  d = e - mu is a subtraction AT THE MAGNITUDE OF mu: within e_mu + u r of the exact d in norm.  r = |d| from an E-long
  fmaf chain and a square root: e_r = e_mu + (E / 2 + 3) u r.  q = (r - dv)^2: e_q = 2 |r - dv| e_r + e_r^2 + 3 u q.
* variance.  sum_p q over n_g terms and the chunks, one division: e_var(g) = (sum e_q + (n_g + chunks + 3) u sum q) / n_g; the labels'
  terms are added over at most L terms: (L + 3) u.
* pairwise.  |mu_i - mu_j| within e_mu(i) + e_mu(j) + (E / 2 + 3) u d_ij; relu is 1-Lipschitz, h = relu(dd - d) within that + u (h + dd);
  h^2 within 2 h e_h + e_h^2 + 2 u h^2; the sum has L terms per label and the labels, blocks and waves above it: (L + 16) u.
* regulariser.  |mu_g| within e_mu + (E / 2 + 2) u |mu_g|, (L + 3) u for the sum.
* the weighted batch sum: (B + 6) u of the magnitudes.

Gradient of pixel p of label g, grad_out (c_g v_p + T_g), v_p = 2 (r - dv) d / r: as a vector, in norm (which bounds every channel):

* v_p.  The length 2 (r - dv) moves by 2 e_r, the direction d / r by at most min(2, 2 e_d / r) (a unit vector under a perturbation
  e_d of d; 2 when r is within the perturbation, r = 0 included, where the reference's gradient is 0 and the fp32 one may have
  any direction): e_v = 2 e_r + 2 |r - dv| min(2, 2 e_d / r) + 8 u |r - dv|.
* c_g = alpha / (B num_id n_g): 4 u.  S_g = sum_p v_p: sum e_v + (n_g + chunks + 1) u sum |v_p|.
* d dist / d mu_i = -2 / (num_id (num_id - 1)) sum_j h_ij (mu_i - mu_j) / d_ij: a term moves by e_h + h min(2, 2 (e_mu(i) + e_mu(j)) / d_ij)
  (coinciding centroids: the reference's 0 against at most 2 h), the sum has L terms: (L + 20) u sum_j h_ij.
* d reg / d mu_g = mu_g / (|mu_g| num_id): min(2, 2 e_mu / |mu_g|) + 4 u, over num_id.
* the products and sums that form T_g and the pixel's gradient: 4 u of each magnitude (7 u where c_g, S_g and n_g meet).
"""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
PARAMS = dict(delta_v=0.5, delta_d=3.0, alpha=1.0, beta=1.0, gama=0.001)
OTHER_PARAMS = dict(delta_v=0.3, delta_d=1.5, alpha=2.0, beta=0.5, gama=0.01)


def chunks(pixels):
    """The split of include/pctrans_hip_train.h: chunks of the pixels of an image."""
    subs = -(-pixels // 256)
    passes = -(-subs // 64)
    return -(-subs // passes)


def clean_labels(labels, L):
    """Labels outside 0 .. L count as background."""
    labels = labels.long()
    return torch.where((labels < 0) | (labels > L), torch.zeros_like(labels), labels)


def loss64(emb, labels, L, delta_v=0.5, delta_d=3.0, alpha=1.0, beta=1.0, gama=0.001, grad_out=1.0):
    """-> (loss, grad [B, E, h, w]) in float64: the reference's loop over the images and their instances."""
    x = emb.detach().cpu().double().requires_grad_(True)
    labels = clean_labels(labels.detach().cpu(), L)
    B, E = x.shape[:2]
    var = dist = reg = x.sum() * 0
    for b in range(B):
        flat, lab = x[b].reshape(E, -1), labels[b].reshape(-1)
        ids = [int(i) for i in torch.unique(lab) if int(i) != 0]
        if not ids:
            continue
        cents = []
        for i in ids:
            mine = flat[:, lab == i]
            mu = mine.mean(1)
            cents.append(mu)
            var = var + (((mine - mu[:, None]).norm(dim=0) - delta_v) ** 2).mean() / len(ids)
        cents = torch.stack(cents)
        if len(ids) > 1:
            d = (cents[:, None, :] - cents[None, :, :]).norm(dim=2) + torch.eye(len(ids), dtype=torch.float64) * delta_d
            dist = dist + (F.relu(delta_d - d) ** 2).sum() / (len(ids) * (len(ids) - 1)) / 2
        reg = reg + cents.norm(dim=1).mean()
    loss = (alpha * var + beta * dist + gama * reg) / B
    grad, = torch.autograd.grad(loss * grad_out, x)
    return float(loss.detach()), grad


def label_map_reference(masks, size):
    """SetCriterion.loss_embedding's label map for a list of [G_i, Ht, Wt] masks, on the masks' device: int64 [B, h, w]."""
    out = []
    for m in masks:
        down = F.interpolate(m[:, None].to(torch.float), size=list(size), mode="nearest")
        down = torch.cat([down.new_zeros((1, 1, size[0], size[1])), down])
        out.append(torch.argmax((down[:, 0] > 0).to(torch.int16), dim=0))
    return torch.stack(out)


def _unit_move(err, length):
    """How far a unit vector can move when its vector of the given length moves by err: min(2, 2 err / length)."""
    return torch.where(length > 0, 2 * err / length.clamp(min=1e-300), torch.full_like(length, 2.0)).clamp(max=2.0)


def bounds(emb, labels, L, delta_v=0.5, delta_d=3.0, alpha=1.0, beta=1.0, gama=0.001, grad_out=1.0):
    """-> (bound on |loss - loss64|, bound [B, 1, h, w] on every channel of |grad - grad64|): the module docstring."""
    x = emb.detach().cpu().double()
    labels = clean_labels(labels.detach().cpu(), L)
    B, E, h, w = x.shape
    P = h * w
    ch = chunks(P)
    a, bt, gm = abs(alpha), abs(beta), abs(gama)
    loss_err, loss_mag = 0.0, 0.0
    gbound = torch.zeros(B, P, dtype=torch.float64)
    for b in range(B):
        flat, lab = x[b].reshape(E, P), labels[b].reshape(P)
        ids = [int(i) for i in torch.unique(lab) if int(i) != 0]
        nid = len(ids)
        if nid == 0:
            continue
        member = torch.stack([lab == i for i in ids]).double()                      # [nid, P]
        n = member.sum(1)
        mu = (member @ flat.t()) / n[:, None]                                       # [nid, E]
        e_mu = ((n + ch + 1)[:, None] * U * (member @ flat.abs().t()) / n[:, None]).norm(dim=1)
        of = member.argmax(0)                                                       # a pixel's row (meaningful inside instances)
        inside = member.sum(0) > 0
        d = flat.t() - mu[of]                                                       # [P, E]
        r = d.norm(dim=1)
        e_d = e_mu[of] + U * r
        e_r = e_mu[of] + (E / 2 + 3) * U * r
        q = (r - delta_v) ** 2
        e_q = 2 * (r - delta_v).abs() * e_r + e_r ** 2 + 3 * U * q
        Q, eQ = member @ (q * inside), member @ (e_q * inside)
        var_g = Q / n
        e_var = ((eQ + (n + ch + 3) * U * Q) / n).sum() / nid + (L + 3) * U * var_g.sum() / nid
        dij = (mu[:, None, :] - mu[None, :, :]).norm(dim=2)
        off = 1 - torch.eye(nid, dtype=torch.float64)
        hij = F.relu(delta_d - dij) * off
        e_dij = e_mu[:, None] + e_mu[None, :] + (E / 2 + 3) * U * dij
        e_h = (e_dij + U * (hij + delta_d)) * off
        dist = (hij ** 2).sum() / max(nid * (nid - 1), 1) / 2
        e_dist = (((2 * hij * e_h + e_h ** 2 + 2 * U * hij ** 2).sum() + (L + 16) * U * (hij ** 2).sum())
                  / max(nid * (nid - 1), 1) / 2 + 3 * U * dist) if nid > 1 else 0.0
        norms = mu.norm(dim=1)
        reg = norms.mean()
        e_reg = (e_mu + (E / 2 + 2) * U * norms).sum() / nid + (L + 3) * U * reg
        loss_err += a * float(e_var) + bt * float(e_dist) + gm * float(e_reg)
        loss_mag += a * float(var_g.sum() / nid) + bt * float(dist) + gm * float(reg)
        # ---- gradient
        c = a / (B * nid * n)                                                       # [nid]
        vlen = 2 * (r - delta_v).abs()
        e_v = 2 * e_r + vlen * _unit_move(e_d, r) + 4 * U * vlen
        sum_v, sum_ev = member @ (vlen * inside), member @ (e_v * inside)
        e_S = sum_ev + (n + ch + 1) * U * sum_v
        e_t1 = (c * e_S + 7 * U * c * sum_v) / n
        if nid > 1:
            move = _unit_move(e_mu[:, None] + e_mu[None, :], dij)
            e_dd = 2.0 / (nid * (nid - 1)) * (((e_h + hij * move) * off).sum(1) + (L + 20) * U * hij.sum(1))
            ddist = 2.0 / (nid * (nid - 1)) * hij.sum(1)                            # at most this long
        else:
            e_dd = ddist = torch.zeros(nid, dtype=torch.float64)
        e_dr = (_unit_move(e_mu, norms) + 4 * U) / nid
        dreg = torch.full_like(norms, 1.0 / nid)
        e_T = e_t1 + (bt * e_dd + gm * e_dr + 4 * U * (bt * ddist + gm * dreg)) / (B * n)
        T_len = c * sum_v / n + (bt * ddist + gm * dreg) / (B * n)
        e_dir = c[of] * e_v + 4 * U * c[of] * vlen
        total = e_dir + e_T[of] + 4 * U * (c[of] * vlen + T_len[of])
        gbound[b] = abs(grad_out) * total * inside
    loss_bound = loss_err / B + (B + 6) * U * loss_mag / B
    return loss_bound, gbound.reshape(B, 1, h, w)


def torch_fp32(emb, labels, params=PARAMS, grad_out=1.0):
    """The criterion's torch formulation in fp32 on the input's device -> (loss, grad)."""
    from pctrans_amd.loss import maskformer_criterion as crit
    x = emb.detach().clone().requires_grad_(True)
    loss = crit.discriminative_loss(x, labels.long(), **params)
    grad, = torch.autograd.grad(loss * grad_out, x)
    return loss.detach(), grad


# ---- inputs: what the GPU tests run, and the CPU tests check the bound on ---------------------------------------------------------
SHAPES = [(16, 13, 11, 1), (3, 67, 61, 31), (32, 13, 11, 33), (16, 67, 61, 70), (32, 67, 61, 33), (3, 13, 11, 70)]   # E, h, w, L
FAMILIES = ("background image", "one instance", "identical instances", "near and far centroids", "offset 100 spread 0.01",
            "all but one pixel")


def exists(name, L):
    """A family needs two instances where it is about a pair of them."""
    return L >= 2 or name not in ("identical instances", "near and far centroids")


def _random_labels(g, P, L, drop=()):
    lab = torch.randint(0, L + 1, (P,), generator=g)
    for k in drop:
        lab[lab == k] = 0
    return lab


@functools.lru_cache(maxsize=None)
def family(name, E, h, w, L, seed=0):
    """-> (emb [2, E, h, w] fp32, labels [2, h, w] int32), both on the CPU.  Cached: treat as read-only."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * E + h + 31 * L + len(name))
    P = h * w
    emb = torch.randn(2, E, P, generator=g)
    lab = torch.stack([_random_labels(g, P, L, drop=(L // 2,) if L > 2 else ()), _random_labels(g, P, max(1, L // 3))])
    if name == "background image":
        lab[0] = 0
    elif name == "one instance":
        lab[0] = (lab[0] > 0).long() * L                      # the last label alone
        lab[1] = (torch.rand(P, generator=g) < 0.3).long()
    elif name == "identical instances":
        # labels 1 and 2: one constant vector of multiples of 1/8 (sums exact: centroids coincide exactly and r_p = 0 exactly);
        # the last two labels: equal up to noise of 1e-6 (centroids coincide to rounding)
        v = torch.randint(-8, 9, (E,), generator=g).float() / 8
        for b in range(2):
            emb[b][:, (lab[b] == 1) | (lab[b] == 2)] = v[:, None]
        if L >= 4:
            base = torch.randn(E, generator=g)
            pick = (lab[0] == L) | (lab[0] == L - 1)
            emb[0][:, pick] = base[:, None] + 1e-6 * torch.randn(E, int(pick.sum()), generator=g)
    elif name == "near and far centroids":
        # centroid of label k at 0.9 k along the first channel: neighbours closer than delta_d = 3, the others farther
        emb = 0.1 * emb
        for b in range(2):
            emb[b, 0] += 0.9 * lab[b].float()
    elif name == "offset 100 spread 0.01":
        emb = 100 + 0.01 * emb
    elif name == "all but one pixel":
        lab[0] = 1
        lab[0, P // 2] = 2 if L >= 2 else 0
    else:
        raise KeyError(name)
    return emb.reshape(2, E, h, w).contiguous(), lab.reshape(2, h, w).to(torch.int32)


@functools.lru_cache(maxsize=None)
def expected(name, E, h, w, L, seed=0):
    """-> (loss64, grad64, loss bound, gradient bound) of a family at the default parameters.  Cached: treat as read-only."""
    emb, lab = family(name, E, h, w, L, seed)
    loss, grad = loss64(emb, lab, L, **PARAMS)
    lb, gb = bounds(emb, lab, L, **PARAMS)
    return loss, grad, lb, gb


def cases():
    return [(name, E, h, w, L) for (E, h, w, L) in SHAPES for name in FAMILIES if exists(name, L)]
