"""TEST INFRASTRUCTURE: plain fp64 formulas of the SeeCoder side (lib/model_zoo/swin.py, seecoder.py, layers.MultiheadAttention) and
of the AutoKL side (autokl_modules.py, autokl.py), deliberately wrong variants of them, and the case table of
tests/test_encoder_vae_blocks_cpu.py / tests/test_encoder_vae_blocks_gpu.py.

Everything follows tests/block_refs.py, whose helpers it imports: the formulas restate the reference's module text (file:line under
the reference project) in the dtype of the parameter view `P`, `wrong=` names ONE composition error (WRONG), the cases are rows of
the same shape as block_refs.CASES and are registered with block_refs so that built() / run_gpu() / ops_standin.run_standin() /
ops_standin.floor() serve them too.  Image blocks take and return NCHW here, token blocks [B, L, C]; the harness at the end converts
to the NHWC / token-major tensors of the product path.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import block_refs as BR
from block_refs import P, Built, _c, _sd, conv2d, layer_norm, linear, nchw, nhwc, rand16, seed_module

WRONG = (
    # swin.py
    "swin_shift_on_even", "swin_mlp_res_from_normed", "swin_attn_res_from_normed", "swin_next_stage_from_out_norm",
    "embed_pad_top_left", "merge_quadrants_swapped",
    # seecoder.py: Decoder
    "dec_levels_fine_first", "dec_level_embed_by_tag_order", "dec_split_lengths_reversed", "dec_seq1_attends_tokens",
    "dec_lateral_from_tokens", "dec_ffn_res_prenorm",
    # seecoder.py: QueryTransformer, layers.MultiheadAttention
    "qt_pos_added_to_value", "qt_globals_cross_attend", "qt_level_cycle_off_by_one", "qt_self_before_cross",
    "qt_cross_result_not_seen_by_self", "qt_qpos_missing_in_self", "qt_level_embed_missing", "mha_pad_keys_unmasked",
    "mha_heads_interleaved",
    # autokl_modules.py, autokl.py
    "vae_eps_1e5", "vae_skip_from_normed", "vae_attn_softmax_over_queries", "vae_attn_scale_missing", "vae_attn_v_of_sample0",
    "vae_attn_res_from_normed", "vae_down_pad_top_left", "vae_up_ceil", "vae_decode_scale_missing", "vae_decode_clamp_before_affine",
    "vae_encode_no_affine")
WS = 12


# ------------------------------------------------------------------------------------------------
# swin.py
# ------------------------------------------------------------------------------------------------
def rel_index(ws):
    """swin.py:155-169: (dy + ws - 1) (2 ws - 1) + (dx + ws - 1) for (query i, key j)"""
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    ys, xs = ys.flatten(), xs.flatten()
    return (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)


def swin_block(p, x, H, W, heads, shift, ws=WS, wrong=None):
    """swin.py:254-310 (block), :178-210 (WindowAttention.forward), :421-440 (the shift mask of BasicLayer.forward).
    x [B, H W, C] -> [B, H W, C]"""
    B, L, Cc = x.shape
    d = Cc // heads
    xn = layer_norm(p.sub("norm1."), x)
    h = xn.view(B, H, W, Cc)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    h = F.pad(h, (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = H + pad_b, W + pad_r
    if shift > 0:
        h = torch.roll(h, shifts=(-shift, -shift), dims=(1, 2))
    nWy, nWx = Hp // ws, Wp // ws
    win = h.view(B, nWy, ws, nWx, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, Cc)
    qkv = linear(p.sub("attn.qkv."), win).reshape(-1, ws * ws, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * d ** -0.5, qkv[1], qkv[2]
    bias = p["attn.relative_position_bias_table"][rel_index(ws).view(-1)].view(ws * ws, ws * ws, heads)
    attn = q @ k.transpose(-2, -1) + bias.permute(2, 0, 1)[None]
    if shift > 0:
        img = torch.zeros((Hp, Wp), dtype=x.dtype)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for ws_ in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[hs, ws_] = cnt
                cnt += 1
        mw = img.view(nWy, ws, nWx, ws).permute(0, 2, 1, 3).reshape(nWy * nWx, ws * ws)
        mask = torch.where(mw[:, None, :] != mw[:, :, None], -100.0, 0.0).to(x.dtype)
        attn = (attn.view(B, nWy * nWx, heads, ws * ws, ws * ws) + mask[None, :, None]).view(-1, heads, ws * ws, ws * ws)
    o = (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(-1, ws * ws, Cc)
    o = linear(p.sub("attn.proj."), o)
    o = o.view(B, nWy, nWx, ws, ws, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, Cc)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    o = o[:, :H, :W].reshape(B, L, Cc)
    x = (xn if wrong == "swin_attn_res_from_normed" else x) + o
    xn2 = layer_norm(p.sub("norm2."), x)
    m = linear(p.sub("mlp.fc2."), F.gelu(linear(p.sub("mlp.fc1."), xn2)))
    return (xn2 if wrong == "swin_mlp_res_from_normed" else x) + m


def patch_embed(p, x, patch=4, wrong=None):
    """swin.py:478-495: zero padding on the right / bottom to a multiple of the patch, patch x patch convolution of that stride,
    LayerNorm where the module has one.  x NCHW -> (tokens [B, Wh Ww, C], Wh, Ww)"""
    _, _, H, W = x.shape
    pr, pb = (patch - W % patch) % patch, (patch - H % patch) % patch
    x = F.pad(x, (pr, 0, pb, 0) if wrong == "embed_pad_top_left" else (0, pr, 0, pb))
    h = conv2d(p.sub("proj."), x, stride=patch)
    Wh, Ww = h.shape[2:]
    t = h.flatten(2).transpose(1, 2)
    if "norm.weight" in p:
        t = layer_norm(p.sub("norm."), t)
    return t, Wh, Ww


def patch_merging(p, x, H, W, wrong=None):
    """swin.py:325-351: pad to even, the 2x2 neighbours in the order (0,0) (1,0) (0,1) (1,1) of (row, column) offsets along the
    channels, LayerNorm(4 C), reduction without bias.  x [B, H W, C] -> [B, ceil(H/2) ceil(W/2), 2 C]"""
    B, L, Cc = x.shape
    g = F.pad(x.view(B, H, W, Cc), (0, 0, 0, W % 2, 0, H % 2))
    quads = [g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]]
    if wrong == "merge_quadrants_swapped":
        quads[1], quads[2] = quads[2], quads[1]
    g = torch.cat(quads, -1).reshape(B, -1, 4 * Cc)
    return linear(p.sub("reduction."), layer_norm(p.sub("norm."), g))


def swin_stage_walk(p, x, embed_dim, depths, heads, out_indices, want=None, wrong=None):
    """swin.py:623-653: patch embedding, per stage the blocks (shift on the odd ones, :385-397), the stage's output LayerNorm for
    the stages in out_indices, PatchMerging of the UN-normalised block output into the next stage.  x NCHW -> {tag: NCHW}"""
    t, Wh, Ww = patch_embed(p.sub("patch_embed."), x, wrong=wrong)
    B = t.shape[0]
    outs = {}
    for i, depth in enumerate(depths):
        dim = embed_dim * 2 ** i
        for j in range(depth):
            odd = j % 2 == (0 if wrong == "swin_shift_on_even" else 1)
            t = swin_block(p.sub(f"layers.{i}.blocks.{j}."), t, Wh, Ww, heads[i], WS // 2 if odd else 0, wrong=wrong)
        o = layer_norm(p.sub(f"norm{i}."), t) if i in out_indices else None
        tag = f"res{i + 2}"
        if o is not None and (want is None or tag in want):
            outs[tag] = o.view(B, Wh, Ww, dim).permute(0, 3, 1, 2)
        if i < len(depths) - 1:
            src = o if (wrong == "swin_next_stage_from_out_norm" and o is not None) else t
            t = patch_merging(p.sub(f"layers.{i}.downsample."), src, Wh, Ww, wrong=wrong)
            Wh, Ww = (Wh + 1) // 2, (Ww + 1) // 2
    return outs


# ------------------------------------------------------------------------------------------------
# nn.MultiheadAttention as seecoder.py builds it, seecoder.py
# ------------------------------------------------------------------------------------------------
def mha(p, q, k, v, heads, wrong=None):
    """torch.nn.MultiheadAttention without batch_first (seecoder.py:70, :110, :160): q [Lq, N, E], k / v [Lk, N, E]; packed
    in_proj, q scaled by d^-1/2, softmax over the keys, out_proj"""
    E = q.shape[-1]
    w, b = p["in_proj_weight"], p["in_proj_bias"]
    qp = F.linear(q, w[:E], b[:E])
    kp = F.linear(k, w[E:2 * E], b[E:2 * E])
    vp = F.linear(v, w[2 * E:], b[2 * E:])
    if wrong == "mha_pad_keys_unmasked":            # the zero columns that pad V^T to 8 keys take part, with a score of 0
        n = (-kp.shape[0]) % 8
        kp, vp = F.pad(kp, (0, 0, 0, 0, 0, n)), F.pad(vp, (0, 0, 0, 0, 0, n))
    Lq, N, _ = qp.shape
    Lk = kp.shape[0]
    d = E // heads
    if wrong == "mha_heads_interleaved":            # head h holds the channels h, h + heads, ... instead of h d .. h d + d - 1
        sp = lambda t, n_: t.reshape(n_, N, d, heads).permute(1, 3, 0, 2).reshape(N * heads, n_, d)  # noqa: E731
    else:
        sp = lambda t, n_: t.reshape(n_, N * heads, d).transpose(0, 1)  # noqa: E731
    qh, kh, vh = sp(qp, Lq) * d ** -0.5, sp(kp, Lk), sp(vp, Lk)
    o = torch.softmax(qh @ kh.transpose(1, 2), dim=-1) @ vh                     # [N heads, Lq, d]
    if wrong == "mha_heads_interleaved":
        o = o.reshape(N, heads, Lq, d).permute(2, 0, 3, 1).reshape(Lq, N, E)
    else:
        o = o.transpose(0, 1).reshape(Lq, N, E)
    return linear(p.sub("out_proj."), o)


def seecoder_decoder_layer(p, x, heads, wrong=None):
    """seecoder.py:81-90 (post-norm): the seq-first attention is handed [B, L, C] (:83), so it attends over the BATCH axis -- for one
    image a softmax over a single key.  x [B, L, C]"""
    if wrong == "dec_seq1_attends_tokens":          # a batch-first attention over the tokens: the reading hip_seq1 rejects
        a = mha(p.sub("self_attn."), x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), heads).transpose(0, 1)
    else:
        a = mha(p.sub("self_attn."), x, x, x, heads)
    pre = x + a
    h = layer_norm(p.sub("norm1."), pre)
    h2 = linear(p.sub("linear2."), F.relu(linear(p.sub("linear1."), h)))
    return layer_norm(p.sub("norm2."), (pre if wrong == "dec_ffn_res_prenorm" else h) + h2)


def seecoder_decoder(p, feats, heads, layers, wrong=None):
    """seecoder.py:394-428, every level a transformer input: per level 1x1 convolution + GroupNorm(32, eps 1e-5) + level embedding
    (indexed by the position in the COARSEST-FIRST order, :398-405), concatenated coarsest first, `layers` DecoderLayers, split by
    the level lengths, + lateral (1x1 convolution without bias, GroupNorm) of the level's own input.  feats {tag: NCHW} ->
    {tag: NCHW}"""
    tags = sorted(feats)
    order = tags[::-1]
    xs, shapes = {}, {}
    for idx, tag in enumerate(order):
        q = p.sub(f"inproj_layers.{tag}.")
        xi = F.group_norm(conv2d(q.sub("0."), feats[tag]), 32, q["1.weight"], q["1.bias"], 1e-5)
        shapes[tag] = xi.shape[-2:]
        e = tags.index(tag) if wrong == "dec_level_embed_by_tag_order" else idx
        xs[tag] = xi.flatten(2).transpose(1, 2) + p["level_embed"][e].view(1, 1, -1)
    cat_order = tags if wrong == "dec_levels_fine_first" else order
    h0 = torch.cat([xs[t] for t in cat_order], 1)
    h = h0
    for i in range(layers):
        h = seecoder_decoder_layer(p.sub(f"transformer.layers.{i}."), h, heads, wrong)
    split_order = tags if wrong == "dec_split_lengths_reversed" else cat_order      # (the running offsets of the other order)
    out, off = {}, {}
    o = 0
    for t in split_order:
        off[t] = o
        o += xs[t].shape[1]
    for tag in tags:
        H, W = shapes[tag]
        src = h0 if wrong == "dec_lateral_from_tokens" else h       # (the lateral joins the tokens in front of the transformer)
        yi = src[:, off[tag]:off[tag] + H * W]
        lat = p.sub(f"lateral_layers.{tag}.")
        l_ = F.group_norm(F.conv2d(feats[tag], lat["weight"]), 32, lat["norm.weight"], lat["norm.bias"], 1e-5)
        out[tag] = yi.transpose(1, 2).reshape(yi.shape[0], -1, H, W) + l_
    return out


def ppe_mlp(p, h, w, freq_num=20, freq_max=None):
    """seecoder.py:285-310: sin / cos of the centred pixel coordinates at freq_num geometric frequencies, three Linears with SiLU
    between them -> tokens [h w, C]"""
    dt = p.dtype
    minlen = min(h, w)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dt), torch.arange(w, dtype=dt), indexing="ij")
    ys = (ys + 0.5 - h / 2) / minlen * 2 * math.pi
    xs = (xs + 0.5 - w / 2) / minlen * 2 * math.pi
    dim_t = (freq_max if freq_max is not None else minlen / 2) ** torch.linspace(0, 1, freq_num, dtype=dt)
    ph, pw = ys[:, :, None] * dim_t, xs[:, :, None] * dim_t
    pos = torch.cat((ph.sin(), ph.cos(), pw.sin(), pw.cos()), dim=-1)
    pos = linear(p.sub("mlp.4."), F.silu(linear(p.sub("mlp.2."), F.silu(linear(p.sub("mlp.0."), pos)))))
    return pos.reshape(h * w, -1)


def cross_layer(p, q, kv, q_pos, k_pos, heads, wrong=None):
    """seecoder.py:171-188 (post-norm): positions join the query and the key, not the value.  q [B, Nq, C], kv [B, Nk, C]"""
    q_in = q if q_pos is None else q + q_pos
    k_in = kv if k_pos is None else kv + k_pos
    v_in = k_in if wrong == "qt_pos_added_to_value" else kv
    h = mha(p.sub("multihead_attn."), q_in.transpose(0, 1), k_in.transpose(0, 1), v_in.transpose(0, 1), heads, wrong).transpose(0, 1)
    return layer_norm(p.sub("norm."), q + h)


def self_layer(p, x, pos, heads, wrong=None, stale=None):
    """seecoder.py:121-133 (post-norm).  stale: what the attention reads in place of x (a variant of query_transformer)"""
    src = x if stale is None else stale
    qk = src if (pos is None or wrong == "qt_qpos_missing_in_self") else src + pos
    h = mha(p.sub("self_attn."), qk.transpose(0, 1), qk.transpose(0, 1), src.transpose(0, 1), heads, wrong).transpose(0, 1)
    return layer_norm(p.sub("norm."), x + h)


def ffn_layer(p, x, wrong=None):
    """seecoder.py:227-232 (post-norm, ReLU)"""
    return layer_norm(p.sub("norm."), x + linear(p.sub("linear2."), F.relu(linear(p.sub("linear1."), x))))


def query_transformer(p, feats, heads, num_gq, layers, wrong=None):
    """seecoder.py:500-550: per level (input projection where the module has one,) + level embedding, positions from the PPE where
    one is attached; per layer the LOCAL queries cross-attend level i mod 3, all queries self-attend, the FFN.  feats: NCHW list
    (res3, res4, res5) -> [B, gq + lq, C]"""
    has_pe = "pe_layer.mlp.0.weight" in p
    fea, pos = [], []
    for i, x in enumerate(feats):
        if f"input_proj.{i}.weight" in p:
            x = conv2d(p.sub(f"input_proj.{i}."), x)
        H, W = x.shape[-2:]
        pos.append(ppe_mlp(p.sub("pe_layer."), H, W)[None] if has_pe else None)
        t = x.flatten(2).transpose(1, 2)
        fea.append(t if wrong == "qt_level_embed_missing" else t + p["level_embed.weight"][i][None, None])
    B = fea[0].shape[0]
    n = len(feats)
    q = p["init_query.weight"][None].repeat(B, 1, 1)
    qp = p["query_pos_embedding.weight"][None].repeat(B, 1, 1)
    for i in range(layers):
        lvl = (i + 1) % n if wrong == "qt_level_cycle_off_by_one" else i % n
        ca, sa = p.sub(f"transformer_crossatt_layers.{i}."), p.sub(f"transformer_selfatt_layers.{i}.")
        lo = 0 if wrong == "qt_globals_cross_attend" else num_gq

        def cross(t):
            return torch.cat([t[:, :lo], cross_layer(ca, t[:, lo:], fea[lvl], qp[:, lo:], pos[lvl], heads, wrong)], 1)
        if wrong == "qt_self_before_cross":
            q = cross(self_layer(sa, q, qp, heads, wrong))
        elif wrong == "qt_cross_result_not_seen_by_self":
            q = self_layer(sa, cross(q), qp, heads, wrong, stale=q)
        else:
            q = self_layer(sa, cross(q), qp, heads, wrong)
        q = ffn_layer(p.sub(f"transformer_feedforward_layers.{i}."), q, wrong)
    return q


# ------------------------------------------------------------------------------------------------
# autokl_modules.py, autokl.py
# ------------------------------------------------------------------------------------------------
def vae_norm(p, x, wrong=None):
    """autokl_modules.py:38-39: GroupNorm(32, eps 1e-6)"""
    return F.group_norm(x, 32, p["weight"], p["bias"], 1e-5 if wrong == "vae_eps_1e5" else 1e-6)


def vae_resnet(p, x, wrong=None):
    """autokl_modules.py:119-141 (temb None)"""
    hn = F.silu(vae_norm(p.sub("norm1."), x, wrong))
    h = conv2d(p.sub("conv1."), hn, padding=1)
    h = conv2d(p.sub("conv2."), F.silu(vae_norm(p.sub("norm2."), h, wrong)), padding=1)
    sk = hn if wrong == "vae_skip_from_normed" else x
    if "nin_shortcut.weight" in p:
        sk = conv2d(p.sub("nin_shortcut."), sk)
    return sk + h


def vae_attn(p, x, wrong=None):
    """autokl_modules.py:176-202: one head over the h w tokens, scale int(C)^-1/2, softmax over the keys"""
    B, Cc, H, W = x.shape
    hn = vae_norm(p.sub("norm."), x, wrong)
    tok = lambda t: t.reshape(B, Cc, H * W).transpose(1, 2)  # noqa: E731
    q, k, v = tok(conv2d(p.sub("q."), hn)), tok(conv2d(p.sub("k."), hn)), tok(conv2d(p.sub("v."), hn))
    if wrong == "vae_attn_v_of_sample0":
        v = v[:1].expand_as(v)
    s = q @ k.transpose(1, 2) * (1.0 if wrong == "vae_attn_scale_missing" else int(Cc) ** (-0.5))
    w = s.softmax(dim=1 if wrong == "vae_attn_softmax_over_queries" else 2)
    o = (w @ v).transpose(1, 2).reshape(B, Cc, H, W)
    return (hn if wrong == "vae_attn_res_from_normed" else x) + conv2d(p.sub("proj_out."), o)


def vae_upsample(p, x, wrong=None):
    """autokl_modules.py:52-57: nearest 2x, conv3x3"""
    if wrong == "vae_up_ceil":
        iy = ((torch.arange(2 * x.shape[2]) + 1) >> 1).clamp(max=x.shape[2] - 1)
        ix = ((torch.arange(2 * x.shape[3]) + 1) >> 1).clamp(max=x.shape[3] - 1)
        up = x[:, :, iy][:, :, :, ix]
    else:
        up = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return conv2d(p.sub("conv."), up, padding=1)


def vae_downsample(p, x, wrong=None):
    """autokl_modules.py:72-79: zero padding of one row / column at the bottom / right, conv3x3 stride 2 without padding"""
    return conv2d(p.sub("conv."), F.pad(x, (1, 0, 1, 0) if wrong == "vae_down_pad_top_left" else (0, 1, 0, 1)), stride=2)


def _levels(p, stem):
    n = 0
    while f"{stem}.{n}.block.0.norm1.weight" in p:
        n += 1
    return n


def _level_blocks(p, stem, lvl):
    n = 0
    while f"{stem}.{lvl}.block.{n}.norm1.weight" in p:
        n += 1
    return n


def vae_encoder(p, x, wrong=None):
    """Encoder.forward autokl_modules.py:432-459; the level / block counts are read off the state dict"""
    h = conv2d(p.sub("conv_in."), x, padding=1)
    nl = _levels(p, "down")
    for lvl in range(nl):
        for b in range(_level_blocks(p, "down", lvl)):
            h = vae_resnet(p.sub(f"down.{lvl}.block.{b}."), h, wrong)
            if f"down.{lvl}.attn.{b}.norm.weight" in p:
                h = vae_attn(p.sub(f"down.{lvl}.attn.{b}."), h, wrong)
        if lvl != nl - 1:
            h = vae_downsample(p.sub(f"down.{lvl}.downsample."), h, wrong)
    h = vae_resnet(p.sub("mid.block_1."), h, wrong)
    h = vae_attn(p.sub("mid.attn_1."), h, wrong)
    h = vae_resnet(p.sub("mid.block_2."), h, wrong)
    return conv2d(p.sub("conv_out."), F.silu(vae_norm(p.sub("norm_out."), h, wrong)), padding=1)


def vae_decoder(p, z, wrong=None):
    """Decoder.forward autokl_modules.py:535-568"""
    h = conv2d(p.sub("conv_in."), z, padding=1)
    h = vae_resnet(p.sub("mid.block_1."), h, wrong)
    h = vae_attn(p.sub("mid.attn_1."), h, wrong)
    h = vae_resnet(p.sub("mid.block_2."), h, wrong)
    nl = _levels(p, "up")
    for lvl in reversed(range(nl)):
        for b in range(_level_blocks(p, "up", lvl)):
            h = vae_resnet(p.sub(f"up.{lvl}.block.{b}."), h, wrong)
            if f"up.{lvl}.attn.{b}.norm.weight" in p:
                h = vae_attn(p.sub(f"up.{lvl}.attn.{b}."), h, wrong)
        if lvl != 0:
            h = vae_upsample(p.sub(f"up.{lvl}.upsample."), h, wrong)
    return conv2d(p.sub("conv_out."), F.silu(vae_norm(p.sub("norm_out."), h, wrong)), padding=1)


def autokl_decode(p, z, in_scale, wrong=None):
    """pfd.py:275-282 (1 / scale_factor * z), autokl.py:44-54 (post_quant_conv, decoder, (dec + 1) / 2 clamped to [0, 1])"""
    if wrong != "vae_decode_scale_missing":
        z = z * in_scale
    h = vae_decoder(p.sub("decoder."), conv2d(p.sub("post_quant_conv."), z), wrong)
    if wrong == "vae_decode_clamp_before_affine":
        return (torch.clamp(h, 0, 1) + 1) / 2
    return torch.clamp((h + 1) / 2, 0, 1)


def autokl_encode_moments(p, x, wrong=None):
    """autokl.py:34-38: x in [0, 1] -> x * 2 - 1 -> encoder -> quant_conv (the moments of the posterior)"""
    if wrong != "vae_encode_no_affine":
        x = x * 2 - 1
    return conv2d(p.sub("quant_conv."), vae_encoder(p.sub("encoder."), x, wrong))


# ------------------------------------------------------------------------------------------------
# cases: Swin
# ------------------------------------------------------------------------------------------------
def _cat(outs, B):
    """several outputs as one [B, total] tensor, in the order of the sorted tags"""
    return torch.cat([outs[k].reshape(B, -1) for k in sorted(outs)], 1)


def build_swin_block(dim=64, nH=2, H=12, W=12, shift=0, B=1, seed=21):
    from lib.model_zoo import swin as SW
    b = Built()
    b.B = B
    b.mods = {"blk": seed_module(SW.SwinTransformerBlock(dim, nH, window_size=WS, shift_size=shift), seed)}
    b.inputs = {"x": rand16((B * H * W, dim), seed + 10, 1.0, 0.3)}
    b.run = lambda m, i: m["blk"].hip(i["x"], B, H, W)
    b.ref = lambda wrong=None, dtype=torch.float64: swin_block(P(_sd(b, "blk"), dtype=dtype), b.inputs["x"].to(dtype).view(B, H * W, dim),
                                                               H, W, nH, shift, wrong=wrong).reshape(B * H * W, dim)
    b.applies = ["swin_mlp_res_from_normed", "swin_attn_res_from_normed"]
    return b


def build_swin_embed(H=50, W=70, norm=True, B=2, seed=23):
    from lib.model_zoo import swin as SW
    b = Built()
    b.B = B
    b.mods = {"pe": seed_module(SW.PatchEmbed(4, 3, 64, norm_layer=nn.LayerNorm if norm else None), seed)}
    b.inputs = {"x": rand16((B, H, W, 3), seed + 10, 0.3, 0.5)}
    b.run = lambda m, i: m["pe"].hip(i["x"])[0]
    b.ref = lambda wrong=None, dtype=torch.float64: patch_embed(P(_sd(b, "pe"), dtype=dtype), nchw(b.inputs["x"].to(dtype)),
                                                                wrong=wrong)[0].reshape(-1, 64)
    b.applies = ["embed_pad_top_left"] if (H % 4 or W % 4) else []
    return b


def build_swin_merge(dim=64, H=13, W=18, B=2, seed=25):
    from lib.model_zoo import swin as SW
    b = Built()
    b.B = B
    b.mods = {"pm": seed_module(SW.PatchMerging(dim), seed)}
    b.inputs = {"x": rand16((B * H * W, dim), seed + 10, 1.0, 0.3)}
    b.run = lambda m, i: m["pm"].hip(i["x"], B, H, W)
    b.ref = lambda wrong=None, dtype=torch.float64: patch_merging(P(_sd(b, "pm"), dtype=dtype), b.inputs["x"].to(dtype).view(B, H * W, dim),
                                                                  H, W, wrong).reshape(-1, 2 * dim)
    b.applies = ["merge_quadrants_swapped"]
    return b


SWIN2 = dict(embed_dim=64, depths=[2, 2], num_heads=[2, 4], window_size=WS, out_indices=(0, 1))
SWIN4 = dict(embed_dim=64, depths=[2, 2, 2, 2], num_heads=[2, 4, 8, 16], window_size=WS, out_indices=(0, 1, 2, 3))


def build_swin_walk(cfg=SWIN2, H=50, W=70, want=None, seed=27):
    from lib.model_zoo import swin as SW
    b = Built()
    b.B = 1
    b.mods = {"net": seed_module(SW.SwinTransformer(**cfg), seed)}
    b.inputs = {"x": rand16((1, H, W, 3), seed + 10, 0.3, 0.5)}
    kw = {} if want is None else {"want": want}
    b.run = lambda m, i: _cat(m["net"].hip(i["x"], **kw), 1)
    if want is None:
        b.fwd = lambda m, i: _cat({k: nhwc(v) for k, v in m["net"].forward(nchw(i["x"]).contiguous()).items()}, 1)

    def ref(wrong=None, dtype=torch.float64):
        outs = swin_stage_walk(P(_sd(b, "net"), dtype=dtype), nchw(b.inputs["x"].to(dtype)), cfg["embed_dim"], cfg["depths"],
                               cfg["num_heads"], cfg["out_indices"], want, wrong)
        return _cat({k: nhwc(v) for k, v in outs.items()}, 1)
    b.ref = ref
    b.applies = ["swin_shift_on_even", "swin_mlp_res_from_normed", "swin_attn_res_from_normed", "embed_pad_top_left",
                 "merge_quadrants_swapped", "swin_next_stage_from_out_norm"]
    return b


# ------------------------------------------------------------------------------------------------
# cases: SeeCoder decoder
# ------------------------------------------------------------------------------------------------
DEC_LEVELS = {"res3": (7, 9, 64), "res4": (4, 5, 128), "res5": (2, 3, 96)}


def build_declayer(L=37, dim=192, seed=31):
    from lib.model_zoo import seecoder as SC
    b = Built()
    b.B = 1
    b.mods = {"lay": seed_module(SC.DecoderLayer(dim=dim, feedforward_dim=256, dropout=0.0, n_heads=8), seed)}
    b.inputs = {"x": rand16((L, dim), seed + 10, 1.0, 0.3)}
    b.run = lambda m, i: m["lay"].hip(i["x"])
    b.ref = lambda wrong=None, dtype=torch.float64: seecoder_decoder_layer(P(_sd(b, "lay"), dtype=dtype), b.inputs["x"].to(dtype)[None], 8, wrong)[0]
    b.applies = ["dec_seq1_attends_tokens", "dec_ffn_res_prenorm"]
    return b


def _decoder(levels, layers, seed):
    from lib.model_zoo import seecoder as SC
    return seed_module(SC.Decoder(inchannels={t: c for t, (_, _, c) in levels.items()}, trans_input_tags=sorted(levels),
                                  trans_num_layers=layers, trans_dim=192, trans_nheads=8, trans_dropout=0.0,
                                  trans_feedforward_dim=256), seed)


def build_decoder(levels=None, layers=2, fwd=True, seed=33):
    levels = dict(DEC_LEVELS if levels is None else levels)
    b = Built()
    b.B = 1
    b.mods = {"dec": _decoder(levels, layers, seed)}
    b.inputs = {t: rand16((1, h, w, c), seed + 10 + n, 1.0, 0.2) for n, (t, (h, w, c)) in enumerate(sorted(levels.items()))}
    b.run = lambda m, i: _cat(m["dec"].hip({t: i[t] for t in levels}), 1)
    if fwd:
        b.fwd = lambda m, i: _cat({k: nhwc(v) for k, v in m["dec"].forward({t: nchw(i[t]).contiguous() for t in levels}).items()}, 1)

    def ref(wrong=None, dtype=torch.float64):
        outs = seecoder_decoder(P(_sd(b, "dec"), dtype=dtype), {t: nchw(b.inputs[t].to(dtype)) for t in levels}, 8, layers, wrong)
        return _cat({k: nhwc(v) for k, v in outs.items()}, 1)
    b.ref = ref
    b.applies = ["dec_levels_fine_first", "dec_level_embed_by_tag_order", "dec_split_lengths_reversed", "dec_seq1_attends_tokens",
                 "dec_lateral_from_tokens", "dec_ffn_res_prenorm"]
    return b


# ------------------------------------------------------------------------------------------------
# cases: MultiheadAttention, the query transformer's layers, the query transformer, the whole encoder
# ------------------------------------------------------------------------------------------------
HID, NH, NGQ, NLQ = 192, 2, 3, 10


def build_mha(Nq=13, Nk=33, self_attn=False, seed=41):
    from lib.hip import layers as L
    b = Built()
    b.B = 1
    b.mods = {"mha": seed_module(L.MultiheadAttention(HID, NH, dropout=0.0), seed)}
    if self_attn:
        b.inputs = {"q": rand16((Nq, HID), seed + 10, 1.0, 0.2)}
        b.inputs.update(k=b.inputs["q"], v=b.inputs["q"], res=b.inputs["q"])
    else:
        b.inputs = {"q": rand16((Nq, HID), seed + 10, 1.0, 0.2), "k": rand16((Nk, HID), seed + 11, 1.0, -0.1),
                    "v": rand16((Nk, HID), seed + 12, 1.0, 0.3), "res": rand16((Nq, HID), seed + 13)}
    b.run = lambda m, i: m["mha"].hip(i["q"], i["k"], i["v"], res=i["res"])

    def ref(wrong=None, dtype=torch.float64):
        i = {k: v.to(dtype) for k, v in b.inputs.items()}
        return mha(P(_sd(b, "mha"), dtype=dtype), i["q"][:, None], i["k"][:, None], i["v"][:, None], NH, wrong)[:, 0] + i["res"]
    b.ref = ref
    b.applies = ["mha_heads_interleaved"] + (["mha_pad_keys_unmasked"] if b.inputs["k"].shape[0] % 8 else [])
    return b


def build_qt_layer(kind="cross", pos=True, seed=43):
    """one layer of the query transformer the way QueryTransformer.hip calls it: the cross-attention writes into a row-offset view
    of the query matrix (the rows in front of it must stay), self-attention and the FFN write over their input"""
    from lib.model_zoo import seecoder as SC
    b = Built()
    b.B = 1
    N = NGQ + NLQ
    cls = {"cross": SC.CrossAttentionLayer, "self": SC.SelfAttentionLayer}.get(kind)
    mod = SC.FeedForwardLayer(HID, 256) if kind == "ffn" else cls(HID, NH)
    b.mods = {"lay": seed_module(mod, seed)}
    b.inputs = {"q": rand16((N, HID), seed + 10, 1.0, 0.2), "qpos": rand16((N, HID), seed + 11, 0.5),
                "kv": rand16((33, HID), seed + 12, 1.0, -0.1), "kpos": rand16((33, HID), seed + 13, 0.5)}

    def run(m, i):
        q = i["q"].clone()
        if kind == "cross":
            lq = q[NGQ:]
            y = m["lay"].hip(lq, i["kv"], q_pos=i["qpos"][NGQ:] if pos else None, k_pos=i["kpos"] if pos else None, out=lq)
            assert y.data_ptr() == lq.data_ptr()
        elif kind == "self":
            m["lay"].hip(q, qk_pos=i["qpos"] if pos else None, out=q)
        else:
            m["lay"].hip(q, out=q)
        return q

    def ref(wrong=None, dtype=torch.float64):
        i = {k: v.to(dtype)[None] for k, v in b.inputs.items()}
        p = P(_sd(b, "lay"), dtype=dtype)
        if kind == "cross":
            y = cross_layer(p, i["q"][:, NGQ:], i["kv"], i["qpos"][:, NGQ:] if pos else None, i["kpos"] if pos else None, NH, wrong)
            return torch.cat([i["q"][:, :NGQ], y], 1)[0]
        if kind == "self":
            return self_layer(p, i["q"], i["qpos"] if pos else None, NH, wrong)[0]
        return ffn_layer(p, i["q"], wrong)[0]
    b.run, b.ref = run, ref
    b.applies = {"cross": ["mha_heads_interleaved", "mha_pad_keys_unmasked"] + (["qt_pos_added_to_value"] if pos else []),
                 "self": ["mha_heads_interleaved", "mha_pad_keys_unmasked"] + (["qt_qpos_missing_in_self"] if pos else []), "ffn": []}[kind]
    return b


def build_ppe(h=5, w=7, seed=45):
    from lib.model_zoo import seecoder as SC
    b = Built()
    b.B = 1
    b.mods = {"pe": seed_module(SC.PPE_MLP(freq_num=20, freq_max=None, out_channel=HID, mlp_layer=3), seed)}
    b.inputs = {}
    b.run = lambda m, i: m["pe"].hip(h, w, next(m["pe"].parameters()).device)
    b.ref = lambda wrong=None, dtype=torch.float64: ppe_mlp(P(_sd(b, "pe"), dtype=dtype), h, w)
    b.applies = []
    return b


def _qt(cin, layers, pa, seed):
    from lib.model_zoo import seecoder as SC
    return seed_module(SC.QueryTransformer(in_channels=cin, hidden_dim=HID, num_queries=[NGQ, NLQ], nheads=NH, num_layers=layers,
                                           feedforward_dim=256, with_fea2d_pos=pa), seed)


def build_qt(cin=HID, layers=4, pa=False, fwd=False, seed=47):
    b = Built()
    b.B = 1
    b.mods = {"qt": _qt(cin, layers, pa, seed)}
    tags = sorted(DEC_LEVELS)
    b.inputs = {t: rand16((1, DEC_LEVELS[t][0], DEC_LEVELS[t][1], cin), seed + 10 + n, 1.0, 0.2) for n, t in enumerate(tags)}
    b.run = lambda m, i: m["qt"].hip([i[t] for t in tags])
    if fwd:
        b.fwd = lambda m, i: m["qt"].forward([nchw(i[t]).contiguous() for t in tags])[0]
    b.ref = lambda wrong=None, dtype=torch.float64: query_transformer(P(_sd(b, "qt"), dtype=dtype), [nchw(b.inputs[t].to(dtype)) for t in tags],
                                                                      NH, NGQ, layers, wrong)[0]
    b.applies = ["qt_globals_cross_attend", "qt_level_cycle_off_by_one", "qt_self_before_cross", "qt_cross_result_not_seen_by_self",
                 "qt_qpos_missing_in_self", "qt_level_embed_missing", "mha_pad_keys_unmasked", "mha_heads_interleaved"] + \
        (["qt_pos_added_to_value"] if pa else [])
    return b


class _Cfg(dict):
    """the two fields and the .get() the model registry reads of a configuration node"""
    __getattr__ = dict.__getitem__


def build_encode_mini(H=100, W=100, depths=(2, 2, 2, 2), seed=49):
    """SemanticContextEncoder over a four-stage Swin at embed_dim 64 (res3..res5: 128 / 256 / 512 channels at 13x13, 7x7, 4x4 for a
    100 x 100 picture: odd merges, the last stage below one window), a two-layer decoder and the four-layer query transformer"""
    from lib.model_zoo import seecoder as SC
    b = Built()
    b.B = 1
    sw = dict(SWIN4, depths=list(depths))
    chans = {"res3": 128, "res4": 256, "res5": 512}
    net = SC.SemanticContextEncoder(
        _Cfg(type="swin", args=dict(sw)),
        _Cfg(type="seecoder_decoder", args=dict(inchannels=chans, trans_input_tags=sorted(chans), trans_num_layers=2, trans_dim=HID,
                                                trans_nheads=8, trans_dropout=0.0, trans_feedforward_dim=256)),
        _Cfg(type="seecoder_query_transformer", args=dict(in_channels=HID, hidden_dim=HID, num_queries=[NGQ, NLQ], nheads=NH,
                                                          num_layers=4, feedforward_dim=256, with_fea2d_pos=False)))
    b.mods = {"net": seed_module(net, seed)}
    b.inputs = {"x": rand16((1, H, W, 3), seed + 10, 0.25, 0.5).clamp(0, 1)}
    b.run = lambda m, i: m["net"].hip(i["x"])
    b.fwd = lambda m, i: m["net"].forward(nchw(i["x"]).contiguous())[0]

    def ref(wrong=None, dtype=torch.float64):
        sd = _sd(b, "net")
        fea = swin_stage_walk(P(sd, "imencoder.", dtype), nchw(b.inputs["x"].to(dtype)), 64, sw["depths"], sw["num_heads"],
                              sw["out_indices"], ("res3", "res4", "res5"), wrong)
        dec = seecoder_decoder(P(sd, "imdecoder.", dtype), fea, 8, 2, wrong)
        return query_transformer(P(sd, "qtransformer.", dtype), [dec["res3"], dec["res4"], dec["res5"]], NH, NGQ, 4, wrong)[0]
    b.ref = ref
    b.applies = []
    return b


# ------------------------------------------------------------------------------------------------
# cases: VAE
# ------------------------------------------------------------------------------------------------
def build_vae_rb(cin=128, cout=None, B=2, H=8, W=8, scale=1.0, shift=0.3, seed=61):
    from lib.model_zoo import autokl_modules as AK
    b = Built()
    b.B = B
    b.mods = {"rb": seed_module(AK.ResnetBlock(in_channels=cin, out_channels=cout, dropout=0.0, temb_channels=0), seed)}
    b.inputs = {"x": rand16((B, H, W, cin), seed + 10, scale, shift)}
    b.run = lambda m, i: m["rb"].hip(i["x"])
    b.ref = lambda wrong=None, dtype=torch.float64: nhwc(vae_resnet(P(_sd(b, "rb"), dtype=dtype), nchw(b.inputs["x"].to(dtype)), wrong))
    b.applies = ["vae_skip_from_normed", "vae_eps_1e5"]
    return b


def build_vae_attn(C=512, B=1, H=8, W=8, seed=63):
    from lib.model_zoo import autokl_modules as AK
    b = Built()
    b.B = B
    b.mods = {"attn": seed_module(AK.AttnBlock(C), seed)}
    b.inputs = {"x": rand16((B, H, W, C), seed + 10, 1.0, 0.3)}
    b.run = lambda m, i: m["attn"].hip(i["x"])
    b.ref = lambda wrong=None, dtype=torch.float64: nhwc(vae_attn(P(_sd(b, "attn"), dtype=dtype), nchw(b.inputs["x"].to(dtype)), wrong))
    b.applies = ["vae_attn_softmax_over_queries", "vae_attn_scale_missing", "vae_attn_res_from_normed"] + \
        (["vae_attn_v_of_sample0"] if B > 1 else [])
    return b


def build_vae_resample(kind="up", C=128, B=2, H=16, W=16, seed=65):
    from lib.model_zoo import autokl_modules as AK
    b = Built()
    b.B = B
    b.mods = {"m": seed_module((AK.Upsample if kind == "up" else AK.Downsample)(C, True), seed)}
    b.inputs = {"x": rand16((B, H, W, C), seed + 10, 1.0, 0.2)}
    b.run = lambda m, i: m["m"].hip(i["x"])
    f = vae_upsample if kind == "up" else vae_downsample
    b.ref = lambda wrong=None, dtype=torch.float64: nhwc(f(P(_sd(b, "m"), dtype=dtype), nchw(b.inputs["x"].to(dtype)), wrong))
    b.applies = ["vae_up_ceil"] if kind == "up" else ["vae_down_pad_top_left"]
    return b


VAE_MINI = dict(double_z=True, z_channels=4, resolution=16, in_channels=3, out_ch=3, ch=128, ch_mult=(1, 4), num_res_blocks=1,
                attn_resolutions=[], dropout=0.0)
IN_SCALE = 1 / 0.18215


def build_vae_mini(kind="dec", dtype16=False, B=2, seed=67):
    """AutoencoderKL at two levels (128 / 512 channels, one block per level, mid attention at the 8 x 8 latent = 64 tokens)
    through .decode(in_scale) / .encode(out_posterior=True).parameters -- the NCHW boundaries are part of the case"""
    from lib.model_zoo import autokl as AKL
    b = Built()
    b.B = B
    b.mods = {"vae": seed_module(AKL.AutoencoderKL(dict(VAE_MINI), None, 4), seed)}
    if kind == "dec":
        z = rand16((B, 4, 8, 8), seed + 10, 0.18215)
        b.inputs = {"z": z if dtype16 else z.float()}
        b.run = lambda m, i: m["vae"].decode(i["z"], in_scale=IN_SCALE)
        b.ref = lambda wrong=None, dtype=torch.float64: autokl_decode(P(_sd(b, "vae"), dtype=dtype), b.inputs["z"].to(dtype), IN_SCALE, wrong)
        if dtype16:      # Decoder.forward: the decoder alone behind the plain boundary kernels
            b.fwd = lambda m, i: m["vae"].decoder.forward(i["z"])
            b.ref_fwd = lambda: vae_decoder(P(_sd(b, "vae"), "decoder."), b.inputs["z"].double())
        b.applies = ["vae_eps_1e5", "vae_skip_from_normed", "vae_attn_softmax_over_queries", "vae_attn_scale_missing",
                     "vae_attn_v_of_sample0", "vae_attn_res_from_normed", "vae_up_ceil", "vae_decode_scale_missing",
                     "vae_decode_clamp_before_affine"]
    else:
        b.inputs = {"x": rand16((B, 3, 16, 16), seed + 11, 0.25, 0.5).clamp(0, 1)}
        b.run = lambda m, i: m["vae"].encode(i["x"], out_posterior=True).parameters
        b.ref = lambda wrong=None, dtype=torch.float64: autokl_encode_moments(P(_sd(b, "vae"), dtype=dtype), b.inputs["x"].to(dtype), wrong)
        b.fwd = lambda m, i: m["vae"].encoder.forward(i["x"])
        b.ref_fwd = lambda: vae_encoder(P(_sd(b, "vae"), "encoder."), b.inputs["x"].double())
        b.applies = ["vae_eps_1e5", "vae_skip_from_normed", "vae_attn_softmax_over_queries", "vae_attn_scale_missing",
                     "vae_attn_v_of_sample0", "vae_attn_res_from_normed", "vae_down_pad_top_left", "vae_encode_no_affine"]
    return b


# ------------------------------------------------------------------------------------------------
# checks both test files run, on their device
# ------------------------------------------------------------------------------------------------
def refusals(dev):
    """[(what, exception, call)]: the calls of this host code that must be refused before the first launch.  Shared by the CPU and
    the GPU file."""
    from lib.model_zoo import swin as SW
    dec = BR._dev(BR.built("see-dec-3lvl"), dev)[0]["dec"]
    qt = BR._dev(BR.built("see-qt-4layer"), dev)[0]["qt"]
    attn = BR._dev(BR.built("vae-attn-512-8x8"), dev)[0]["attn"]
    see = BR._dev(BR.built("see-encode-mini"), dev)[0]["net"]
    feats2 = {t: BR.rand16((2, h, w, c), 3).to(dev) for t, (h, w, c) in DEC_LEVELS.items()}
    lv = [BR.rand16((b, h, w, 192), 4).to(dev) for b in (1, 2) for (h, w, _) in (DEC_LEVELS[t] for t in sorted(DEC_LEVELS))]
    wa = BR.seed_module(SW.WindowAttention(64, 7, 2), 5).half().to(dev)
    blk = BR.seed_module(SW.SwinTransformerBlock(64, 2, window_size=7, shift_size=3), 6).half().to(dev)
    t49 = BR.rand16((49, 64), 7).to(dev)
    return [("Decoder.hip B 2", NotImplementedError, lambda: dec.hip(feats2)),
            ("QueryTransformer.hip B 2", NotImplementedError, lambda: qt.hip(lv[3:])),
            ("QueryTransformer.hip two levels", AssertionError, lambda: qt.hip(lv[:2])),
            ("AttnBlock.hip 48 tokens", NotImplementedError, lambda: attn.hip(BR.rand16((1, 6, 8, 512), 8).to(dev))),
            ("WindowAttention.hip window 7", NotImplementedError, lambda: wa.hip(t49, 1, 7, 7, 0, t49)),
            ("SwinTransformerBlock.hip window 7", NotImplementedError, lambda: blk.hip(t49, 1, 7, 7)),
            ("SemanticContextEncoder.hip B 2", NotImplementedError, lambda: see.hip(BR.rand16((2, 100, 100, 3), 9, 0.2, 0.5).to(dev)))]


def ppe_cache_check(pe, dev):
    """PPE_MLP.features caches per shape: the same shape twice, then two shapes alternating -- the third call equals the first in
    bits, and the table is the cached object.  Shared by the CPU and the GPU file."""
    a1 = pe.hip(5, 7, dev).clone()
    t1 = pe.features(5, 7, dev)
    a2 = pe.hip(5, 7, dev).clone()
    assert pe.features(5, 7, dev) is t1 and torch.equal(a1, a2)
    b1 = pe.hip(6, 6, dev).clone()
    a3 = pe.hip(5, 7, dev).clone()
    b2 = pe.hip(6, 6, dev).clone()
    assert pe.features(5, 7, dev) is t1 and len(pe._feat_cache) == 2
    assert torch.equal(a3, a1) and torch.equal(b2, b1) and a1.shape == (35, HID) and b1.shape == (36, HID)
    return a1, b1



_GEMM = {"PFD_VAE_ATTN": "gemm", "AttnBlock.ROWS": 128}
# branch: the census token(s) the case is written for, as in block_refs.CASES
CASES = [
    # ---- Swin ----
    _c("swin-blk-64-12x12-s0", "swin", "swin_window_attention", build_swin_block),
    _c("swin-blk-64-12x12-s6", "swin", "swin_window_attention", build_swin_block, shift=6),
    _c("swin-blk-64-13x18-s6-b2", "swin", "swin_window_attention", build_swin_block, H=13, W=18, shift=6, B=2),
    _c("swin-blk-128-5x7-s6", "swin", "swin_window_attention", build_swin_block, dim=128, nH=4, H=5, W=7, shift=6),
    _c("swin-embed-50x70", "swin", "conv_narrow layernorm", build_swin_embed),
    _c("swin-embed-48x48-nonorm", "swin", "conv_narrow", build_swin_embed, sep=False, H=48, W=48, norm=False),
    _c("swin-merge-13x18", "swin", "layernorm_patch_merge gemm[]", build_swin_merge),
    _c("swin-walk-2stage", "swin", "layernorm_patch_merge", build_swin_walk, forward=True),
    _c("swin-walk-2stage-res3", "swin", "layernorm_patch_merge", build_swin_walk, want=("res3",)),
    # ---- SeeCoder decoder ----
    _c("see-declayer-192", "seedec", "gemm[] gemm[res] layernorm gemm[relu] gemm[res] layernorm", build_declayer),
    _c("see-dec-3lvl", "seedec", "conv_narrow groupnorm add_rowvec[out] gemm[] groupnorm add_rowvec[out]", build_decoder, forward=True),
    _c("see-dec-3lvl-1token", "seedec", "conv_narrow groupnorm add_rowvec[out]", build_decoder, fwd=False,
       levels={"res3": (7, 9, 64), "res4": (4, 5, 128), "res5": (1, 1, 96)}),
    # ---- MultiheadAttention, query transformer ----
    _c("see-mha-13q-33k", "qt", "gemm[bpr,out] attention gemm[res]", build_mha),
    _c("see-mha-self-13", "qt", "gemm[bpr,out] attention gemm[res]", build_mha, self_attn=True),
    _c("see-cross-layer", "qt", "add add gemm[] gemm[] gemm[bpr,out] attention gemm[res] layernorm[out]", build_qt_layer),
    _c("see-cross-layer-nopos", "qt", "gemm[] gemm[] gemm[bpr,out] attention gemm[res] layernorm[out]", build_qt_layer, pos=False),
    _c("see-self-layer", "qt", "add gemm[] gemm[] gemm[bpr,out] attention gemm[res] layernorm[out]", build_qt_layer, kind="self"),
    _c("see-ffn-layer", "qt", "gemm[relu] gemm[res] layernorm[out]", build_qt_layer, sep=False, kind="ffn"),
    _c("see-ppe-5x7", "qt", "gemm[silu] gemm[silu] gemm[]", build_ppe, sep=False),
    _c("see-ppe-6x6", "qt", "gemm[silu] gemm[silu] gemm[]", build_ppe, sep=False, h=6, w=6),
    _c("see-qt-4layer", "qt", "add_rowvec add_rowvec add_rowvec add gemm[]", build_qt, forward=True, fwd=True),
    _c("see-qt-4layer-pa", "qt", "gemm[silu] gemm[silu] gemm[] add add", build_qt, pa=True),
    _c("see-qt-inproj", "qt", "gemm[] add_rowvec gemm[] add_rowvec", build_qt, cin=128),
    _c("see-encode-mini", "qt", "swin_window_attention", build_encode_mini, sep=False, forward=True),
    # ---- VAE ----
    _c("vae-rb-128", "vae", "groupnorm conv[] groupnorm conv[res]", build_vae_rb),
    _c("vae-rb-128-256-nin", "vae", "gemm[] conv[res]", build_vae_rb, cout=256, H=9, W=7),
    _c("vae-rb-512", "vae", "groupnorm conv[] groupnorm conv[res]", build_vae_rb, cin=512),
    _c("vae-rb-128-smallvar", "vae", "groupnorm conv[] groupnorm conv[res]", build_vae_rb, scale=0.01, shift=0.0),
    _c("vae-attn-512-8x8", "vae", "gemm[bpr] attention gemm[res]", build_vae_attn),
    _c("vae-attn-512-8x16-b2", "vae", "gemm[bpr] attention gemm[res]", build_vae_attn, B=2, W=16),
    _c("vae-attn-512-gemm-12x16-rows128", "vae", "gemm[out] softmax_rows[out] gemm[out] gemm[out] softmax_rows[out] gemm[out]",
       build_vae_attn, switches=_GEMM, B=2, H=12, W=16),
    _c("vae-attn-256-gemm", "vae", "gemm[out] softmax_rows[out] gemm[out]", build_vae_attn, C=256, B=2),
    _c("vae-up-128-16", "vae", "conv[ups=2:served", build_vae_resample),
    _c("vae-up-512-8", "vae", "conv[ups=2:declined", build_vae_resample, C=512, H=8, W=8),
    _c("vae-down-16", "vae", "conv[ohw,s2", build_vae_resample, kind="down"),
    _c("vae-down-9x7", "vae", "conv[ohw,s2", build_vae_resample, kind="down", H=9, W=7),
    _c("vae-dec-mini", "vae", "to_nhwc conv_narrow", build_vae_mini),
    _c("vae-dec-mini-f16", "vae", "to_nhwc conv_narrow", build_vae_mini, sep=False, forward=True, dtype16=True),
    _c("vae-enc-mini", "vae", "to_nhwc conv_narrow", build_vae_mini, forward=True, kind="enc"),
]
CLASSES = ("swin", "seedec", "qt", "vae")
BR.register(CASES)
