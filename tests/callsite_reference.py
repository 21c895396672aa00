"""Plain-torch definitions of the head's HIP entry points, evaluated on the operands a call actually received
(tests/callsite_capture.py).  `dtype=torch.float64` is the reference; the same definition in float32 is the fp32 yardstick
(run it with TF32 off).  bf16 operands are widened as they are: the reference sees the bf16 values the kernel read.
The `*_autocast` functions are the bf16 yardsticks: what torch computes under bf16 autocast on the same inputs."""
import torch
from torch.nn import functional as F

F64 = torch.float64


def _w(t, dtype):
    return None if t is None else t.detach().to(dtype)


def _layer_norm(y, norm, dtype):
    return F.layer_norm(y, tuple(norm.normalized_shape), _w(norm.weight, dtype), _w(norm.bias, dtype), norm.eps)


# ---------------------------------------------------------------- GEMM epilogues (encoder)
def linear(x, lin, relu=False, x_add=None, dtype=F64):
    """[relu]((x + x_add) W^T + b)"""
    x = x.to(dtype)
    if x_add is not None:
        x = x + x_add.to(dtype)
    y = F.linear(x, _w(lin.weight, dtype), _w(lin.bias, dtype))
    return torch.relu(y) if relu else y


def linear_k128_multi(x, layers, x_add=None, dtype=F64):
    return [linear(x, lin, x_add=x_add if use_add else None, dtype=dtype) for lin, use_add in layers]


def linear_add_layer_norm(x, lin, residual, norm, dtype=F64):
    """LN(residual + x W^T + b)"""
    return _layer_norm(residual.to(dtype) + linear(x, lin, dtype=dtype), norm, dtype)


def ffn_layer_norm(x, linear1, linear2, norm, dtype=F64):
    """LN(x + W2 relu(W1 x + b1) + b2)"""
    return _layer_norm(x.to(dtype) + linear(linear(x, linear1, relu=True, dtype=dtype), linear2, dtype=dtype), norm, dtype)


# ---------------------------------------------------------------- 1x1 convolutions, GroupNorm, flatten
def conv1x1(x, conv, dtype=F64):
    """sum_k W[o, k] x[n, k, h, w] + b[o].  float64: the sum as written; float32: torch's convolution (the yardstick)."""
    if dtype == torch.float32:
        return F.conv2d(x.float(), _w(conv.weight, dtype), _w(conv.bias, dtype))
    w = _w(conv.weight, dtype).reshape(conv.out_channels, -1)
    y = torch.einsum("ok,nkp->nop", w, x.to(dtype).flatten(2)).reshape(x.shape[0], -1, *x.shape[2:])
    return y if conv.bias is None else y + _w(conv.bias, dtype)[None, :, None, None]


def groupnorm_flatten(y, gn, dtype=F64):
    """GroupNorm(y).flatten(2).transpose(1, 2): [N, C, H, W] -> [N, H*W, C]"""
    z = F.group_norm(y.to(dtype), gn.num_groups, _w(gn.weight, dtype), _w(gn.bias, dtype), gn.eps)
    return z.flatten(2).transpose(1, 2)


def conv1x1_groupnorm_tokens(x, conv, gn, dtype=F64):
    return groupnorm_flatten(conv1x1(x, conv, dtype), gn, dtype)


# ---------------------------------------------------------------- MSDeformAttn
def msda(value, spatial_shapes, sampling_loc, attn_weight, dtype=F64):
    from pctrans_amd.pixel_decoder.ops.functions import ms_deform_attn_core_pytorch
    return ms_deform_attn_core_pytorch(value.to(dtype), spatial_shapes, sampling_loc.to(dtype), attn_weight.to(dtype))


def pixel_coords(sampling_loc, spatial_shapes, dtype=F64):
    """(x, y) = loc * (W_l, H_l) - 0.5 per level: [N, Lq, M, L, P, 2].  In float64 this is exact for fp32 locations."""
    wh = torch.stack([spatial_shapes[:, 1], spatial_shapes[:, 0]], -1).to(dtype=dtype, device=sampling_loc.device)
    return sampling_loc.to(dtype) * wh[:, None, :] - 0.5


def msda_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, dtype=F64,
                  delta=1e-4):
    """The sampling op's backward as the reference states it (ops/src/cuda/ms_deform_im2col_cuda.cuh:92-164): a sample
    counts when -1 < y < H and -1 < x < W, each of its four corners when it lies on the map, with the bilinear weights of
    the cell `floor(x), floor(y)`.  -> (grad_value [N, S, M, D], grad_loc [N, Lq, M, L, P, 2, 2], grad_attn [N, Lq, M, L, P]).

    grad_value and grad_attn are continuous in the locations; grad_loc is not: it jumps where a coordinate crosses an
    integer (the cell changes) and at the gate (-1 and H).  So grad_loc[..., c, :] holds two candidates for coordinate c:
    where that coordinate is within `delta` px of an integer k, the derivatives of the cells on either side of k (floor
    k - 1 and floor k, each evaluated at the coordinate itself; a side beyond the gate gives 0), else the single derivative
    twice.  The other coordinate keeps its own cell and gate.  `delta=0` gives the plain derivative (the fp32 yardstick)."""
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_loc.shape
    dev = value.device
    vflat = value.to(dtype).reshape(N * S * M, D)
    attn = attn_weight.to(dtype)
    go = grad_output.to(dtype).reshape(N, Lq, M, 1, D)                       # broadcast over the points
    xy = pixel_coords(sampling_loc, spatial_shapes, dtype)
    grad_value = torch.zeros(N * S * M, D, dtype=dtype, device=dev)
    grad_loc = torch.zeros(N, Lq, M, L, P, 2, 2, dtype=dtype, device=dev)
    grad_attn = torch.zeros(N, Lq, M, L, P, dtype=dtype, device=dev)
    n_idx = torch.arange(N, device=dev).view(N, 1, 1, 1)
    m_idx = torch.arange(M, device=dev).view(1, 1, M, 1)
    for l, (H, W) in enumerate(spatial_shapes.tolist()):
        start = int(level_start_index[l])
        x, y = xy[:, :, :, l, :, 0], xy[:, :, :, l, :, 1]                    # [N, Lq, M, P]
        a = attn[:, :, :, l, :, None]                                         # [N, Lq, M, P, 1]

        def cell(fx, fy, live):
            """-> (value, d value / dx, d value / dy) [N, Lq, M, P, D] of the cell with corner (fx, fy), zero where not
            `live`, and the corners (index, weight, on the map) for the scatter."""
            lx, ly = (x - fx)[..., None], (y - fy)[..., None]
            hx, hy = 1 - lx, 1 - ly
            v, corners = [], []
            for dy in (0, 1):
                for dx in (0, 1):
                    r, c = fy + dy, fx + dx
                    ok = live & (r >= 0) & (r < H) & (c >= 0) & (c < W)
                    idx = ((n_idx * S + start + r.clamp(0, H - 1) * W + c.clamp(0, W - 1)) * M + m_idx).long()
                    v.append(torch.where(ok[..., None], vflat[idx], 0))
                    corners.append((idx, ok, (ly if dy else hy) * (lx if dx else hx)))
            v00, v01, v10, v11 = v
            val = hy * hx * v00 + hy * lx * v01 + ly * hx * v10 + ly * lx * v11
            d_dx = hy * (v01 - v00) + ly * (v11 - v10)
            d_dy = hx * (v10 - v00) + lx * (v11 - v01)
            return val, d_dx, d_dy, corners

        gx, gy = (x > -1) & (x < W), (y > -1) & (y < H)
        fx0, fy0 = torch.floor(x).long(), torch.floor(y).long()
        val, d_dx, d_dy, corners = cell(fx0, fy0, gx & gy)
        gg = go * a                                                           # d out / d sampled value
        grad_attn[:, :, :, l] = (go * val).sum(-1)
        for idx, ok, w in corners:
            contrib = (w * gg).expand(*idx.shape, D)
            grad_value.index_add_(0, idx[ok], contrib[ok])
        for axis, (t, f0, size, gate, other) in enumerate(((x, fx0, W, gx, gy), (y, fy0, H, gy, gx))):
            k = torch.round(t)
            near = (t - k).abs() < delta if delta > 0 else torch.zeros_like(gate)
            for side, f in enumerate((torch.where(near, k.long() - 1, f0), torch.where(near, k.long(), f0))):
                live = torch.where(near, (f >= -1) & (f <= size - 1), gate) & other
                _, ddx, ddy, _ = cell(f, fy0, live) if axis == 0 else cell(fx0, f, live)
                grad_loc[:, :, :, l, :, axis, side] = size * (gg * (ddx if axis == 0 else ddy)).sum(-1)
    return grad_value.reshape(N, S, M, D), grad_loc, grad_attn


def msda_fused(value, spatial_shapes, reference_points, sampling_offsets, attention_logits, dtype=F64):
    """softmax over L*P, ref + off / (W, H), then the sampling op"""
    N, Lq, M, L, P, _ = sampling_offsets.shape
    w = torch.softmax(attention_logits.to(dtype).reshape(N, Lq, M, L * P), -1).reshape(N, Lq, M, L, P)
    wh = torch.stack([spatial_shapes[:, 1], spatial_shapes[:, 0]], -1).to(dtype)            # (W_l, H_l)
    loc = reference_points.to(dtype)[:, :, None, :, None, :] + sampling_offsets.to(dtype) / wh[None, None, None, :, None, :]
    return msda(value, spatial_shapes, loc, w, dtype)


# ---------------------------------------------------------------- dynamic mask head
def mask_head_logits(feats, ref_xy, params, stride, rel_coord, dtype=F64):
    """The three dynamic 1x1 layers as mask_heads_forward_batched states them: feats [N, C, H, W], ref_xy [N, Q, 2]
    normalised (x, y), params [N, Q, G] = [w0 (8 x (2 + C): rel_x, rel_y, feat...) | w1 (8 x 8) | w2 (1 x 8) | b0 | b1 | b2]
    -> [N, Q, H, W]."""
    N, C, H, W = feats.shape
    Q = params.shape[1]
    cin = C + 2 if rel_coord else C
    p = params.to(dtype)
    w0, w1, w2, b0, b1, b2 = torch.split_with_sizes(p, [8 * cin, 64, 8, 8, 8, 1], dim=2)
    w0, w1, w2 = w0.reshape(N, Q, 8, cin), w1.reshape(N, Q, 8, 8), w2.reshape(N, Q, 1, 8)
    f = feats.to(dtype).reshape(N, 1, C, H * W)
    if rel_coord:
        inst = ref_xy.to(dtype) * torch.tensor([W * stride, H * stride], dtype=dtype, device=feats.device)
        ys, xs = torch.meshgrid(torch.arange(H, device=feats.device), torch.arange(W, device=feats.device), indexing="ij")
        loc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).to(dtype) * stride + stride // 2     # pixel centres (x, y)
        rel = inst[:, :, None, :] - loc[None, None]                                                 # [N, Q, HW, 2]
        x = w0[..., 2:] @ f + w0[..., 0:1] * rel[:, :, None, :, 0] + w0[..., 1:2] * rel[:, :, None, :, 1]
    else:
        x = w0 @ f
    x = torch.relu(x + b0[..., None])
    x = torch.relu(w1 @ x + b1[..., None])
    return (w2 @ x + b2[..., None]).reshape(N, Q, H, W)


def mask_head_resize(logits, target_size):
    """-> (x2 bilinear upsample [N, Q, 2H, 2W], bilinear resize to the attention-mask target [N, Q, th*tw]); the mask is
    `sigmoid(resized) < 0.5`, i.e. resized < 0."""
    H, W = logits.shape[-2:]
    up = F.interpolate(logits, size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
    rs = F.interpolate(logits, size=tuple(int(s) for s in target_size), mode="bilinear", align_corners=False)
    return up, rs.flatten(2)


def mask_head(feats, ref_xy, params, stride, rel_coord, target_size, dtype=F64):
    return mask_head_resize(mask_head_logits(feats, ref_xy, params, stride, rel_coord, dtype), target_size)


def mask_head_autocast(feats, ref_xy, params, stride, target_size):
    """bf16 yardstick: the bf16 chain of test_dyn_mask_head_gpu (features, generated weights and hidden activations rounded
    to bf16 as bf16 1x1 convolutions see them; fp32 accumulation, rel-coord term and biases), with the third layer's
    operands rounded too -- the chain there keeps w2 and its input in fp32, where autocast (and the bf16 kernels, which run
    that layer on the matrix cores: csrc/dmh_common.hpp, DmhPair) round both -- then the logits rounded to bf16
    and resized as torch resizes a bf16 tensor."""
    N, C, H, W = feats.shape
    r = lambda t: t.bfloat16().float()
    p = params.float()
    w0, w1, w2, b0, b1, b2 = torch.split_with_sizes(p, [8 * (C + 2), 64, 8, 8, 8, 1], dim=2)
    Q = p.shape[1]
    w0, w1, w2 = w0.reshape(N, Q, 8, C + 2), w1.reshape(N, Q, 8, 8), w2.reshape(N, Q, 1, 8)
    f = r(feats.float()).reshape(N, 1, C, H * W)
    inst = ref_xy.float() * torch.tensor([W * stride, H * stride], dtype=torch.float32, device=feats.device)
    ys, xs = torch.meshgrid(torch.arange(H, device=feats.device), torch.arange(W, device=feats.device), indexing="ij")
    loc = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).float() * stride + stride // 2
    rel = inst[:, :, None, :] - loc[None, None]
    x = r(w0[..., 2:]) @ f + w0[..., 0:1] * rel[:, :, None, :, 0] + w0[..., 1:2] * rel[:, :, None, :, 1] + b0[..., None]
    x = r(torch.relu(x))
    x = r(torch.relu(r(w1) @ x + b1[..., None]))
    lb = (r(w2) @ x + b2[..., None]).reshape(N, Q, H, W).bfloat16()
    return mask_head_resize(lb, target_size)


# ---------------------------------------------------------------- attention
def _mask4(mask, N, L, S):
    if mask is None:
        return None
    return mask.reshape(1, 1, L, S) if mask.dim() == 2 else mask.reshape(N, 1, L, S)


def attention(q, k, v, heads, mask=None, dtype=F64):
    """softmax(mask(q k^T / sqrt(d))) v per head: q [L, N, E], k [S, N, E], v [S, N, Ev], mask bool (True = may not
    attend) [N, 1, L, S] | [L, S].  A fully masked row is NaN (the softmax of all minus infinity)."""
    L, N, E = q.shape
    S, Ev = k.shape[0], v.shape[2]
    hd, vd = E // heads, Ev // heads
    qh = q.to(dtype).reshape(L, N, heads, hd).permute(1, 2, 0, 3)
    kh = k.to(dtype).reshape(S, N, heads, hd).permute(1, 2, 3, 0)
    vh = v.to(dtype).reshape(S, N, heads, vd).permute(1, 2, 0, 3)
    s = (qh @ kh) * hd ** -0.5
    m = _mask4(mask, N, L, S)
    if m is not None:
        s = s.masked_fill(m, float("-inf"))
    return (torch.softmax(s, -1) @ vh).permute(2, 0, 1, 3).reshape(L, N, Ev)


def attention_autocast(q, k, v, heads, mask=None):
    """bf16 yardstick: the decoder's torch formulation (transformer_decoder/attention.py) under bf16 autocast -- scores
    from bf16 operands, softmax in fp32, P rounded to bf16 before P.V."""
    L, N, E = q.shape
    S, Ev = k.shape[0], v.shape[2]
    hd, vd = E // heads, Ev // heads
    with torch.autocast("cuda", dtype=torch.bfloat16):
        qh = (q * float(hd) ** -0.5).reshape(L, N, heads, hd).permute(1, 2, 0, 3)
        kh = k.reshape(S, N, heads, hd).permute(1, 2, 3, 0)
        vh = v.reshape(S, N, heads, vd).permute(1, 2, 0, 3)
        s = torch.matmul(qh, kh)
        m = _mask4(mask, N, L, S)
        if m is not None:
            s = s.masked_fill(m, float("-inf"))
        p = F.softmax(s, dim=-1)
        out = torch.matmul(p, vh)
    return out.permute(2, 0, 1, 3).reshape(L, N, Ev)


def cross_operands(q_content, q_pos, k_content, k_pos, heads, attn_mask=None, row_open=None):
    """The per-head [content | position] concatenations and the mask with the `row_open` rows cleared."""
    def cat(a, b):
        T, N, C = a.shape
        return torch.cat([a.reshape(T, N, heads, C // heads), b.reshape(T, N, heads, C // heads)], 3).reshape(T, N, 2 * C)
    m = attn_mask
    if m is not None and row_open is not None:
        N, L = q_content.shape[1], q_content.shape[0]
        m = m.reshape(N, 1, L, -1) & ~row_open.reshape(N, 1, L, 1)
    return cat(q_content, q_pos), cat(k_content, k_pos), m
