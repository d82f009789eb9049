"""TEST INFRASTRUCTURE: plain fp64 formulas of the UNet blocks, deliberately wrong variants of them, and the case table of
tests/test_blocks_cpu.py / tests/test_blocks_gpu.py.

The formulas restate the reference's module text (file:line under the reference project, the way oracle/pfd_oracle.py cites it)
with F.conv2d / F.group_norm / F.layer_norm / F.linear / softmax in the dtype of the parameter view `P` (fp64 for the tests, fp32
for the pin against oracle/pfd_oracle.py).  They read a module's state dict, so the parameter names are the reference's.

`wrong=` names ONE composition error (WRONG); the formula then computes what a host layer with that error would.  The tests show
that every such variant lies far outside the tolerance: a reference that cannot tell them apart checks nothing.

Image blocks take and return NCHW here; the harness at the end converts to the NHWC / token-major tensors of the product path.
"""
import copy
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

WRONG = (
    "skip_from_normed", "emb_other_sample", "emb_after_norm2", "concat_swapped", "skip_x_only", "ups_ceil", "down_pad_wrong_side",
    "res_other_half", "zero_rows_get_cond", "cond_rows_get_bias", "ctx_sample0", "pad_unmasked", "norm2_affine_for_norm3",
    "ln_stats_160", "geglu_swapped", "no_res_attn1", "no_res_attn2", "no_res_ff", "proj_out_res_after_proj_in", "skip_block2",
    "skip_fifo", "control_to_h", "mix_unnormalised")


class P:
    """prefix view over a state dict, values in `dtype` (oracle/pfd_oracle.py's SD with a dtype)"""

    def __init__(self, sd, prefix="", dtype=torch.float64):
        self.sd, self.prefix, self.dtype = sd, prefix, dtype

    def __getitem__(self, k):
        return self.sd[self.prefix + k].detach().cpu().to(self.dtype)

    def __contains__(self, k):
        return (self.prefix + k) in self.sd

    def sub(self, p):
        return P(self.sd, self.prefix + p, self.dtype)

    def get(self, k):
        return self[k] if k in self else None


def conv2d(p, x, stride=1, padding=0):
    return F.conv2d(x, p["weight"], p.get("bias"), stride=stride, padding=padding)


def linear(p, x):
    w = p["weight"]
    return F.linear(x, w.reshape(w.shape[0], -1), p.get("bias"))


def group_norm(p, x, eps):
    return F.group_norm(x, 32, p["weight"], p["bias"], eps)


def layer_norm(p, x, eps=1e-5, wrong=None):
    if wrong == "ln_stats_160":          # the statistics of the first 160-column slice only
        v = x[..., :160]
        mean = v.mean(-1, keepdim=True)
        var = (v * v).mean(-1, keepdim=True) - mean * mean
        return (x - mean) / torch.sqrt(var + eps) * p["weight"] + p["bias"]
    return F.layer_norm(x, (x.shape[-1],), p["weight"], p["bias"], eps)


# ------------------------------------------------------------------------------------------------
# openaimodel.py
# ------------------------------------------------------------------------------------------------
def res_block(p, x, semb, x2=None, wrong=None):
    """openaimodel.py:254-274 (use_scale_shift_norm=False, no up / down; GroupNorm32 eps 1e-5) over `torch.cat([h, skip], 1)`
    (pfd.py:356).  semb = SiLU(emb): emb_layers is SiLU -> Linear (:217-223)"""
    xin = x if x2 is None else torch.cat([x2, x] if wrong == "concat_swapped" else [x, x2], 1)
    hn = F.silu(group_norm(p.sub("in_layers.0."), xin, 1e-5))
    h = conv2d(p.sub("in_layers.2."), hn, padding=1)
    e = linear(p.sub("emb_layers.1."), semb)
    if wrong == "emb_other_sample":
        e = e.roll(1, 0)
    e = e[:, :, None, None]
    if wrong == "emb_after_norm2":
        g = F.silu(group_norm(p.sub("out_layers.0."), h, 1e-5) + e)
    else:
        g = F.silu(group_norm(p.sub("out_layers.0."), h + e, 1e-5))
    h = conv2d(p.sub("out_layers.3."), g, padding=1)
    sk = hn if wrong == "skip_from_normed" else xin
    if "skip_connection.weight" in p:
        w = p["skip_connection.weight"]
        if wrong == "skip_x_only" and x2 is not None:
            sk = F.conv2d(sk[:, :x.shape[1]], w[:, :x.shape[1]], p.get("skip_connection.bias"), padding=w.shape[-1] // 2)
        else:
            sk = conv2d(p.sub("skip_connection."), sk, padding=w.shape[-1] // 2)
    return sk + h


def upsample(p, x, wrong=None):
    """openaimodel.py:108-117: F.interpolate(scale_factor=2, mode='nearest') then conv3x3"""
    if wrong == "ups_ceil":
        iy = ((torch.arange(2 * x.shape[2]) + 1) >> 1).clamp(max=x.shape[2] - 1)
        ix = ((torch.arange(2 * x.shape[3]) + 1) >> 1).clamp(max=x.shape[3] - 1)
        up = x[:, :, iy][:, :, :, ix]
    else:
        up = F.interpolate(x, scale_factor=2, mode="nearest")
    return conv2d(p.sub("conv."), up, padding=1)


def downsample(p, x, wrong=None):
    """openaimodel.py:149-159: conv3x3, stride 2, padding 1"""
    if wrong == "down_pad_wrong_side":
        return conv2d(p.sub("op."), F.pad(x, (0, 2, 0, 2)), stride=2)
    return conv2d(p.sub("op."), x, stride=2, padding=1)


# ------------------------------------------------------------------------------------------------
# attention.py
# ------------------------------------------------------------------------------------------------
def cross_attention(p, x, context, heads, wrong=None):
    """attention.py:178-201: q / k / v without bias, (q k^T) d^-1/2, softmax, to_out.  x [B, N, C], context [B, Nk, Cc] | None"""
    ctx = x if context is None else context
    if context is not None and wrong == "ctx_sample0":
        ctx = ctx[:1].expand_as(ctx)
    if context is not None and wrong == "pad_unmasked":      # the zero rows that pad the context to 8 tokens take part
        ctx = F.pad(ctx, (0, 0, 0, (-ctx.shape[1]) % 8))
    q, k, v = linear(p.sub("to_q."), x), linear(p.sub("to_k."), ctx), linear(p.sub("to_v."), ctx)
    B, N, Cd = q.shape
    d = Cd // heads
    sp = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = sp(q), sp(k), sp(v)
    attn = ((q @ k.transpose(-1, -2)) * d ** -0.5).softmax(dim=-1)
    return linear(p.sub("to_out.0."), (attn @ v).permute(0, 2, 1, 3).reshape(B, N, Cd))


def attention_branch(p, pn, x, res, context, heads, zero_lead=0, wrong=None):
    """`attn(norm(x), context) + res` (attention.py:303-304) with the variants that concern the CFG batch: the first zero_lead
    samples have an all-zero context (app.py:236)"""
    xn = x if pn is None else layer_norm(pn, x, wrong=wrong)
    y = cross_attention(p, xn, context, heads, wrong)
    B = x.shape[0]
    r = res
    if wrong == "res_other_half":
        r = res.roll(B // 2, 0)
    out = y + r
    z = zero_lead
    if wrong == "zero_rows_get_cond" and 0 < z < B:
        out = out.clone()
        out[:z] = y[B - z:] + r[:z]
    if wrong == "cond_rows_get_bias" and z < B:
        out = out.clone()
        out[z:] = r[z:] + p["to_out.0.bias"]
    return out


def feed_forward(p, x, glu=True, wrong=None):
    """attention.py:44-71: GEGLU (x * gelu(gate)) or Linear + GELU, then Linear"""
    if glu:
        a, gate = linear(p.sub("net.0.proj."), x).chunk(2, dim=-1)
        if wrong == "geglu_swapped":
            a, gate = gate, a
        h = a * F.gelu(gate)
    else:
        h = F.gelu(linear(p.sub("net.0.0."), x))
    return linear(p.sub("net.2."), h)


def basic_transformer_block(p, x, context, heads, disable_self_attn=False, glu=True, zero_lead=0, wrong=None):
    """attention.py:302-306"""
    c1 = context if disable_self_attn else None
    w1 = wrong if wrong in ("ln_stats_160",) or disable_self_attn else None
    y = attention_branch(p.sub("attn1."), p.sub("norm1."), x, x, c1, heads, zero_lead if disable_self_attn else 0, w1)
    x = y - x if wrong == "no_res_attn1" else y
    w2 = None if wrong == "ln_stats_160" else wrong
    y = attention_branch(p.sub("attn2."), p.sub("norm2."), x, x, context, heads, zero_lead, w2)
    x = y - x if wrong == "no_res_attn2" else y
    n3 = p.sub("norm2." if wrong == "norm2_affine_for_norm3" else "norm3.")
    y = feed_forward(p.sub("ff."), layer_norm(n3, x), glu, wrong)
    return y if wrong == "no_res_ff" else y + x


def spatial_transformer(p, x, context, heads, depth=1, disable_self_attn=False, glu=True, zero_lead=0, wrong=None):
    """attention.py:352-371: GroupNorm(eps 1e-6) -> proj_in (1x1 conv, or Linear on the tokens) -> blocks -> proj_out -> + x"""
    B, Cc, H, W = x.shape
    h = group_norm(p.sub("norm."), x, 1e-6).flatten(2).transpose(1, 2)
    h = linear(p.sub("proj_in."), h)
    h_in = h
    for d in range(depth):
        if d == 1 and wrong == "skip_block2":
            continue
        h = basic_transformer_block(p.sub(f"transformer_blocks.{d}."), h, context, heads, disable_self_attn, glu, zero_lead, wrong)
    h = linear(p.sub("proj_out."), h)
    r = x.flatten(2).transpose(1, 2)
    if wrong == "proj_out_res_after_proj_in":
        r = h_in
    return (h + r).transpose(1, 2).reshape(B, -1, H, W)


# ------------------------------------------------------------------------------------------------
# the UNetModel2D_Next walk of pfd.apply_model
# ------------------------------------------------------------------------------------------------
def timestep_embedding(t, dim, dtype, max_period=10000):
    """diffusion_utils.py:131-151 (cos half first)"""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=dtype) / half)
    args = t[:, None].to(dtype) * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def unet(net, p, x, t, contexts, heads, control=None, zero_lead=0, wrong=None):
    """pfd.py:314-365 and :466-528 (control) / :366-386 ('attention' mixing) over the i_order / m_order / o_order lists of
    openaimodel.py:2664-2739.  `net` supplies only those lists and which kind of layer each data block holds; contexts =
    [(P of the net that owns the context blocks, context [B, Nk, Cc], ratio)]"""
    from lib.model_zoo import openaimodel as OM
    emb = linear(p.sub("time_embed.2."), F.silu(linear(p.sub("time_embed.0."), timestep_embedding(t, net.model_channels, p.dtype))))
    semb = F.silu(emb)
    di, ci = [0], [0]

    def data(h, x2=None):
        i = di[0]
        di[0] += 1
        q, m = p.sub(f"data_blocks.{i}.0."), net.data_blocks[i][0]
        if isinstance(m, OM.ResBlock):
            return res_block(q, h, semb, x2)
        if isinstance(m, OM.Downsample):
            return downsample(q, h)
        if isinstance(m, OM.Upsample):
            return upsample(q, h)
        if isinstance(m, nn.Sequential):
            return conv2d(q.sub("2."), F.silu(group_norm(q.sub("0."), h, 1e-5)), padding=1)
        return conv2d(q, h, padding=1)

    def ctx(h):
        i = ci[0]
        ci[0] += 1
        tot = 1.0 if wrong == "mix_unnormalised" else sum(r for _, _, r in contexts)
        return sum(spatial_transformer(pc.sub(f"context_blocks.{i}.0."), h, c, heads, zero_lead=zero_lead) * (r / tot)
                   for pc, c, r in contexts)
    ccs = list(control) if control is not None else None
    hs, h = [], x
    for lt in net.i_order:
        if lt == "d":
            h = data(h)
        elif lt == "c":
            h = ctx(h)
        else:
            hs.append(h)
    for lt in net.m_order:
        h = data(h) if lt == "d" else ctx(h)
    if ccs is not None:
        h = h + ccs.pop()
    skip = None
    for lt in net.o_order:
        if lt == "load_hidden_feature":
            skip = hs.pop()
            if wrong == "skip_fifo":      # the OLDEST saved feature of that shape (a plain FIFO pop does not even fit the first concat)
                hs.append(skip)
                skip = hs.pop(next(n for n, s_ in enumerate(hs) if s_.shape == skip.shape))
            if ccs is not None:
                c = ccs.pop()
                if wrong == "control_to_h" and c.shape == h.shape:
                    h = h + c
                else:
                    skip = skip + c
        elif lt == "d":
            h, skip = data(h, skip), None
        else:
            h = ctx(h)
    return h


# ------------------------------------------------------------------------------------------------
# weights, inputs, the error measure
# ------------------------------------------------------------------------------------------------
def seed_module(mod, seed):
    """every weight from a seeded generator at 1 / sqrt(fan_in) -- the zero-initialised last convolutions and proj_out too (a zero
    branch hides every error inside it); norm gamma 1 + 0.2 n, beta and biases 0.1 n; fp16-representable values in fp32"""
    g = torch.Generator().manual_seed(seed)
    norms = {n for n, m in mod.named_modules() if isinstance(m, (nn.GroupNorm, nn.LayerNorm))}
    with torch.no_grad():
        for name, prm in sorted(mod.named_parameters()):
            owner = name.rsplit(".", 1)[0] if "." in name else ""
            r = torch.randn(prm.shape, generator=g)
            if owner in norms:
                v = 1 + 0.2 * r if name.endswith("weight") else 0.1 * r
            elif prm.dim() >= 2:
                v = r / math.sqrt(prm[0].numel())
            else:
                v = 0.1 * r
            prm.copy_(v.half().float())
    return mod.eval()


def rand16(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).half()


def err_units(y, ref, B):
    """per sample: max_e |y_e - ref_e| / (|ref_e| + rms(ref over the sample)), in units of 2^-11; the largest sample's"""
    y, ref = y.detach().cpu().double().reshape(B, -1), ref.detach().cpu().double().reshape(B, -1)
    rms = ref.pow(2).mean(1, keepdim=True).sqrt()
    return float(((y - ref).abs() / (ref.abs() + rms)).max() * 2.0 ** 11)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
SWITCHES = {"LN_FOLD": ("ops", "LN_FOLD"), "GN_PSTATS": ("ops", "GN_PSTATS"), "GEMM_FUSE": ("ops", "GEMM_FUSE"),
            "UPS_FOLD": ("ops", "UPS_FOLD"), "fuse_groupnorm": ("ResBlock", "fuse_groupnorm"),
            "fuse_reduce_groupnorm": ("ResBlock", "fuse_reduce_groupnorm"), "pair_without_copies": ("ST", "pair_without_copies"),
            "PFD_VAE_ATTN": ("env", "PFD_VAE_ATTN"), "AttnBlock.ROWS": ("AttnBlock", "ROWS")}


def apply_switches(monkeypatch, sw):
    from lib.hip import ops
    from lib.model_zoo import attention as AT, autokl_modules as AK, openaimodel as OM
    owner = {"ops": ops, "ResBlock": OM.ResBlock, "ST": AT.SpatialTransformer, "AttnBlock": AK.AttnBlock}
    monkeypatch.delenv("PFD_VAE_ATTN", raising=False)          # (a case runs the form it names, whatever the caller's environment)
    for k, v in (sw or {}).items():
        o, a = SWITCHES[k]
        if o == "env":
            monkeypatch.setenv(a, v)
        else:
            monkeypatch.setattr(owner[o], a, v)


class Built:
    """one case, built: .mods (CPU modules holding fp16 values), .inputs, .B, .run(mods, inputs) through the real .hip methods on
    whatever device they live on, .ref(wrong, dtype) the formula (same layout as .run's result), .applies the variants that change
    this case's formula"""


def _dev(b, device):
    mods = {k: copy.deepcopy(m).half().to(device) for k, m in b.mods.items()}
    inputs = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in b.inputs.items()}
    return mods, inputs


def run_case(b, device):
    """the case through the real host layer on `device` (the stand-in has to be installed for 'cpu') -> CPU tensor"""
    mods, inputs = _dev(b, device)
    return b.run(mods, inputs).detach().cpu()


def _sd(b, name):
    return {k: v.half() for k, v in b.mods[name].state_dict().items()}


def build_resblock(c1=320, c2=0, cout=320, B=2, H=8, W=8, use_conv=False, emb="semb", chain=None, heads=8, seed=1):
    from lib.hip import ops
    from lib.model_zoo import attention as AT, openaimodel as OM
    b = Built()
    E = 1280
    b.B = B
    b.mods = {"rb": seed_module(OM.ResBlock(c1 + c2, E, 0.0, out_channels=cout, use_conv=use_conv), seed)}
    if chain in ("res", "ctrl"):
        b.mods["next"] = seed_module(OM.ResBlock(cout, E, 0.0, out_channels=cout), seed + 1)
    if chain == "st":
        b.mods["next"] = seed_module(AT.SpatialTransformer(cout, heads, cout // heads, context_dim=768), seed + 1)
    b.inputs = {"x": rand16((B, H, W, c1), seed + 10, 1.0, 0.3), "semb": rand16((B, E), seed + 11, 0.5)}
    if c2:
        b.inputs["x2"] = rand16((B, H, W, c2), seed + 12, 0.7, -0.2)
    if chain == "ctrl":
        b.inputs["ctrl"] = rand16((B, H, W, cout), seed + 13, 0.5)
    if chain == "st":
        b.inputs["ctx"] = rand16((B, 20, 768), seed + 14)

    def run(m, i):
        rb, nxt = m["rb"], m.get("next")
        blocks = [rb] + ([nxt] if chain in ("res", "ctrl") else [])
        semb, e = i["semb"], None
        if emb != "semb":      # the precomputed projections: one table for every ResBlock, each at its column offset
            rows = semb[:1] if emb == "shared" else semb
            parts, cols, off = [rows[:, :64].contiguous()], {}, 64
            for blk in blocks:
                parts.append(blk.emb_layers[1].hip(rows))
                cols[id(blk)] = off
                off += blk.out_channels
            e, semb = (torch.cat(parts, 1).contiguous(), cols, emb == "shared"), None
        nn_ = None
        if chain in ("res", "ctrl"):
            nn_ = (nxt.in_layers[0], True)
        elif chain == "st":
            nn_ = (nxt.norm, False)
        h = rb.hip(i["x"], semb, x2=i.get("x2"), emb=e, next_norm=nn_)
        if chain == "ctrl":      # ControlNet-style: modified in place through views, sample by sample
            for s in range(B):
                ops.add(h[s:s + 1], i["ctrl"][s:s + 1], out=h[s:s + 1])
        if chain in ("res", "ctrl"):
            h = nxt.hip(h, semb, emb=e)
        elif chain == "st":
            h = nxt.hip(h, AT.ContextKV(i["ctx"]))
        return h

    def ref(wrong=None, dtype=torch.float64):
        i = b.inputs
        semb = i["semb"].to(dtype)
        if emb == "shared":
            semb = semb[:1].expand_as(semb)
        x2 = None if not c2 else nchw(i["x2"].to(dtype))
        h = res_block(P(_sd(b, "rb"), dtype=dtype), nchw(i["x"].to(dtype)), semb, x2, wrong)
        if chain == "ctrl":
            h = h + nchw(i["ctrl"].to(dtype))
        if chain in ("res", "ctrl"):
            h = res_block(P(_sd(b, "next"), dtype=dtype), h, semb)
        elif chain == "st":
            h = spatial_transformer(P(_sd(b, "next"), dtype=dtype), h, i["ctx"].to(dtype), heads)
        return nhwc(h)
    b.run, b.ref = run, ref
    if chain is None and not c2 and emb == "semb":      # the reference calling convention: NCHW, the raw embedding
        b.fwd = lambda m, i: nhwc(m["rb"].forward(nchw(i["x"]).contiguous(), i["semb"]))
        b.ref_fwd = lambda: nhwc(res_block(P(_sd(b, "rb")), nchw(b.inputs["x"].double()), F.silu(b.inputs["semb"].double())))
    b.applies = ["skip_from_normed", "emb_after_norm2"] + (["emb_other_sample"] if emb != "shared" else []) + \
        (["concat_swapped"] if c2 else []) + (["skip_x_only"] if c2 and not use_conv else [])
    return b


def build_resample(kind="up", C=320, B=2, H=16, W=16, seed=3):
    from lib.model_zoo import openaimodel as OM
    b = Built()
    b.B = B
    mod = OM.Upsample(C, True) if kind == "up" else OM.Downsample(C, True)
    b.mods = {"m": seed_module(mod, seed)}
    b.inputs = {"x": rand16((B, H, W, C), seed + 10, 1.0, 0.2)}
    b.run = lambda m, i: m["m"].hip(i["x"])
    b.fwd = lambda m, i: nhwc(m["m"].forward(nchw(i["x"]).contiguous()))
    f = upsample if kind == "up" else downsample
    b.ref = lambda wrong=None, dtype=torch.float64: nhwc(f(P(_sd(b, "m"), dtype=dtype), nchw(b.inputs["x"].to(dtype)), wrong))
    b.applies = ["ups_ceil"] if kind == "up" else ["down_pad_wrong_side"]
    return b


def _context(i, zero_lead):
    from lib.model_zoo import attention as AT
    if "ctx" not in i:
        return None
    kv = AT.ContextKV(i["ctx"])
    kv.zero_lead = zero_lead
    return kv


def _ctx_input(B, Nk, zero_lead, seed):
    c = rand16((B, Nk, 768), seed)
    c[:zero_lead] = 0
    return c


def build_attention(dim=320, heads=8, d_head=40, B=2, N=64, Nk=None, zero_lead=0, fold=True, stats_out=True, single=False, seed=5):
    """CrossAttention.hip with its LayerNorm and residual: `attn(norm(x), context) + x`"""
    from lib.hip import layers as L, ops
    from lib.model_zoo import attention as AT
    b = Built()
    b.B = B
    b.mods = {"attn": seed_module(AT.CrossAttention(dim, 768 if Nk else None, heads, d_head), seed), "norm": seed_module(L.LayerNorm(dim), seed + 1)}
    Bx = B // 2 if single else B
    b.inputs = {"x": rand16((Bx * N, dim), seed + 10, 1.0, 0.3)}
    if Nk:
        b.inputs["ctx"] = _ctx_input(B, Nk, zero_lead, seed + 11)

    def run(m, i):
        attn, norm, x = m["attn"], m["norm"], i["x"]
        kv = _context(i, zero_lead)
        if fold:
            y = attn.hip(x, B, N, kv, res=x, ln=(norm, ops.ln_rowstats(x)), stats_out=stats_out, single=single)
        else:
            y = attn.hip(norm.hip(x), B, N, kv, res=x, stats_out=stats_out)
        if isinstance(y, tuple):
            b.ln_carried = (y[0].detach().cpu(), y[1].detach().cpu())      # (stored tokens, their partial row sums): checked by the tests
            y = y[0]
        return y

    def ref(wrong=None, dtype=torch.float64):
        x = b.inputs["x"].to(dtype).reshape(Bx, N, dim)
        if single:
            x = torch.cat([x, x])
        ctx = b.inputs["ctx"].to(dtype) if Nk else None
        return attention_branch(P(_sd(b, "attn"), dtype=dtype), P(_sd(b, "norm"), dtype=dtype), x, x, ctx, heads, zero_lead,
                                wrong).reshape(B * N, dim)
    b.run, b.ref = run, ref
    if Nk and not zero_lead:                             # CrossAttention.forward: the attention alone, no norm, no residual
        b.fwd = lambda m, i: m["attn"].forward(i["x"].view(B, N, dim), i["ctx"]).reshape(B * N, dim)
        b.ref_fwd = lambda: cross_attention(P(_sd(b, "attn")), b.inputs["x"].double().reshape(B, N, dim), b.inputs["ctx"].double(),
                                            heads).reshape(B * N, dim)
    b.applies = (["ln_stats_160"] if dim > 160 else []) + (["res_other_half"] if not single else [])
    if Nk:
        b.applies += ["ctx_sample0"] + (["pad_unmasked"] if Nk % 8 else [])
        if 0 < zero_lead < B:
            b.applies += ["zero_rows_get_cond", "cond_rows_get_bias"]
    return b


def build_btb(dim=320, heads=8, d_head=40, B=2, N=64, Nk=20, zero_lead=0, disable_self_attn=False, glu=True, seed=7):
    from lib.model_zoo import attention as AT
    b = Built()
    b.B = B
    b.mods = {"blk": seed_module(AT.BasicTransformerBlock(dim, heads, d_head, context_dim=768, gated_ff=glu,
                                                          disable_self_attn=disable_self_attn), seed)}
    b.inputs = {"x": rand16((B * N, dim), seed + 10, 1.0, 0.3), "ctx": _ctx_input(B, Nk, zero_lead, seed + 11)}
    b.run = lambda m, i: m["blk"].hip(i["x"], B, N, _context(i, zero_lead))
    if not zero_lead:
        b.fwd = lambda m, i: m["blk"].forward(i["x"].view(B, N, dim), i["ctx"]).reshape(B * N, dim)

    def ref(wrong=None, dtype=torch.float64):
        x = b.inputs["x"].to(dtype).reshape(B, N, dim)
        return basic_transformer_block(P(_sd(b, "blk"), dtype=dtype), x, b.inputs["ctx"].to(dtype), heads, disable_self_attn, glu,
                                       zero_lead, wrong).reshape(B * N, dim)
    b.ref = ref
    b.applies = ["norm2_affine_for_norm3", "ln_stats_160", "no_res_attn1", "no_res_attn2", "no_res_ff", "ctx_sample0",
                 "res_other_half"] + (["geglu_swapped"] if glu else []) + (["pad_unmasked"] if Nk % 8 else [])
    if 0 < zero_lead < B:
        b.applies += ["zero_rows_get_cond", "cond_rows_get_bias"]
    return b


def build_st(C=320, heads=8, d_head=None, B=2, H=8, W=8, Nk=20, depth=1, use_linear=False, zero_lead=0, cfg_pair=False, seed=9):
    from lib.model_zoo import attention as AT
    b = Built()
    b.B = B
    b.mods = {"st": seed_module(AT.SpatialTransformer(C, heads, d_head or C // heads, depth=depth, context_dim=[768] * depth,
                                                      use_linear=use_linear), seed)}
    Bx = B // 2 if cfg_pair else B
    b.inputs = {"x": rand16((Bx, H, W, C), seed + 10, 1.0, 0.3), "ctx": _ctx_input(B, Nk, zero_lead, seed + 11)}
    b.run = lambda m, i: m["st"].hip(i["x"], _context(i, zero_lead), cfg_pair=cfg_pair)
    if not zero_lead and not cfg_pair:
        b.fwd = lambda m, i: nhwc(m["st"].forward(nchw(i["x"]).contiguous(), i["ctx"]))

    def ref(wrong=None, dtype=torch.float64):
        x = nchw(b.inputs["x"].to(dtype))
        if cfg_pair:
            x = torch.cat([x, x])
        return nhwc(spatial_transformer(P(_sd(b, "st"), dtype=dtype), x, b.inputs["ctx"].to(dtype), heads, depth,
                                        zero_lead=zero_lead, wrong=wrong))
    b.ref = ref
    b.applies = (["proj_out_res_after_proj_in"] if d_head is None else []) + ["no_res_ff", "geglu_swapped", "ctx_sample0"] + (["skip_block2"] if depth == 2 else []) + \
        (["zero_rows_get_cond", "cond_rows_get_bias", "res_other_half"] if 0 < zero_lead < B else [])
    return b


def build_unet(mode="plain", B=2, seed=11):
    """the smallest UNetModel2D_Next with two levels, one ResBlock per level, attention at both, a straddling (640 + 320) and a
    whole-group (320 + 320, 640 + 640) skip concat: model channels 320, channel_mult (1, 2), 16x16 latent"""
    from lib.model_zoo import attention as AT, openaimodel as OM
    b = Built()
    b.B = B
    kw = dict(in_channels=4, model_channels=320, out_channels=4, num_res_blocks=1, attention_resolutions=(1, 2), context_dim=768,
              channel_mult=(1, 2), num_heads=8)
    b.mods = {"net": seed_module(OM.UNetModel2D_Next(**kw), seed)}
    if mode == "mix":
        b.mods["net2"] = seed_module(OM.UNetModel2D_Next(parts=["context"], **kw), seed + 1)
    pair = mode == "cfg_pair"
    z = B // 2 if pair else 0
    Bx = B // 2 if pair else B
    t = torch.tensor([500] * B if mode in ("cfg_pair", "emb_table") else [500, 37][:B])
    b.inputs = {"x": rand16((Bx, 16, 16, 4), seed + 10), "t": t, "ctx": _ctx_input(B, 20, z, seed + 11)}
    if mode == "mix":
        b.inputs["ctx2"] = rand16((B, 77, 768), seed + 12)
    if mode == "control":
        shapes = [(16, 320), (16, 320), (8, 320), (8, 640), (8, 640)]
        for n, (s, c) in enumerate(shapes):
            b.inputs[f"c{n}"] = rand16((B, s, s, c), seed + 20 + n, 0.5)
    ratios = (0.7, 0.8)

    def run(m, i):
        net = m["net"]
        kv = _context(i, z)
        if mode == "mix":
            kv = AT.ContextMix([(net, kv, ratios[0]), (m["net2"], AT.ContextKV(i["ctx2"]), ratios[1])])
        ctrl = [i[f"c{n}"] for n in range(5)] if mode == "control" else None
        tab = net.emb_projections(i["t"][:1])[0] if mode == "emb_table" else None
        return net.hip(i["x"], i["t"], kv, control=ctrl, emb_table=tab, cfg_pair=pair)

    def ref(wrong=None, dtype=torch.float64):
        i = b.inputs
        x = nchw(i["x"].to(dtype))
        if pair:
            x = torch.cat([x, x])
        p = P(_sd(b, "net"), dtype=dtype)
        ctxs = [(p, i["ctx"].to(dtype), 1.0)]
        if mode == "mix":
            ctxs = [(p, i["ctx"].to(dtype), ratios[0]), (P(_sd(b, "net2"), dtype=dtype), i["ctx2"].to(dtype), ratios[1])]
        ctrl = [nchw(i[f"c{n}"].to(dtype)) for n in range(5)] if mode == "control" else None
        return nhwc(unet(b.mods["net"], p, x, i["t"], ctxs, 8, ctrl, z, wrong))
    b.run, b.ref = run, ref
    if mode == "plain":
        b.fwd = lambda m, i: nhwc(m["net"].forward(nchw(i["x"]).contiguous(), i["t"], i["ctx"]))
    b.applies = ["skip_fifo"] + (["control_to_h"] if mode == "control" else []) + (["mix_unnormalised"] if mode == "mix" else [])
    return b


def _c(cid, cls, branch, build, sep=True, switches=None, forward=False, **kw):
    return dict(id=cid, cls=cls, branch=branch, build=build, kw=kw, sep=sep, switches=switches or {}, forward=forward)


# branch: the census token(s) the case is written for (tests assert the case's census line contains them, in this order)
CASES = [
    # ---- ResBlock ----
    _c("rb-identity-320", "resblock", "conv[res", build_resblock, forward=True),
    _c("rb-1x1-320-640", "resblock", "gemm[k]", build_resblock, cout=640),
    _c("rb-3x3skip", "resblock", "conv[]", build_resblock, cout=640, use_conv=True),
    _c("rb-cat-320+320-a2", "resblock", "gemm[a2,k]", build_resblock, c1=320, c2=320, cout=320),
    _c("rb-cat-640+320-straddle", "resblock", "gemm[a2,k]", build_resblock, c1=640, c2=320, cout=320),
    # (160 + 160 -> 320 has as many channels in as out: the constructor gives it the identity skip, which takes no concat)
    _c("rb-cat-160+160-materialised", "resblock", "cat", build_resblock, c1=160, c2=160, cout=640),
    _c("rb-cat-320+320-two-gemm", "resblock", "gemm[res,k,out]", build_resblock, switches={"GEMM_FUSE": False}, c1=320, c2=320, cout=320),
    _c("rb-1280-gnfuse", "resblock", "conv[gnf=", build_resblock, sep=False, c1=1280, cout=1280, B=4),
    _c("rb-1280-next-res", "resblock", "normed_hit", build_resblock, sep=False, c1=1280, cout=1280, B=4, chain="res"),
    _c("rb-1280-next-st", "resblock", "normed_hit", build_resblock, sep=False, c1=1280, cout=1280, B=4, chain="st"),
    _c("rb-1280-ctrl-between", "resblock", "add[out]", build_resblock, sep=False, c1=1280, cout=1280, B=4, chain="ctrl"),
    _c("rb-w32-prologue", "resblock", "conv[gn", build_resblock, switches={"fuse_groupnorm": True}, B=1, H=8, W=32),
    _c("rb-w32-prologue-x2", "resblock", "conv[gn", build_resblock, switches={"fuse_groupnorm": True}, B=1, H=8, W=32, c1=320, c2=320),
    _c("rb-emb-table", "resblock", "conv[rv", build_resblock, emb="table"),
    _c("rb-emb-shared", "resblock", "rpv=2^30", build_resblock, emb="shared"),
    # ---- Upsample / Downsample ----
    _c("up-16-fold", "resample", "conv[ups=2:served", build_resample, kind="up", forward=True),
    _c("up-16-nofold", "resample", "conv[ups=1", build_resample, switches={"UPS_FOLD": False}, kind="up"),
    _c("up-8-declined", "resample", "conv[ups=2:declined", build_resample, kind="up", H=8, W=8),
    _c("up-8-nofold", "resample", "conv[ups=1", build_resample, switches={"UPS_FOLD": False}, kind="up", H=8, W=8),
    _c("down-16", "resample", "conv[s2,gno]", build_resample, kind="down"),
    _c("down-9x7", "resample", "conv[s2]", build_resample, kind="down", H=9, W=7),
    # ---- CrossAttention ----
    _c("attn-self-fused-folded", "attention", "gemm[ln,ot", build_attention),
    _c("attn-self-fused-unfolded", "attention", "gemm[ot", build_attention, fold=False),
    _c("attn-self-inner384", "attention", "gemm[bpr", build_attention, dim=384, heads=4, d_head=96, fold=False, stats_out=False),
    _c("attn-self-odd-3x5", "attention", "gemm[bpr,k,out]", build_attention, N=15, fold=False),
    _c("attn-cross-z0", "attention", "gemm[ln]", build_attention, forward=True, Nk=20),
    _c("attn-cross-zhalf", "attention", "gemm[res,out,zr,lno]", build_attention, Nk=20, zero_lead=1),
    _c("attn-cross-zall", "attention", "gemm[ln] attention gemm[res,lno]", build_attention, Nk=20, zero_lead=2),
    _c("attn-cross-zhalf-nostats", "attention", "gemm[res,out,zr]", build_attention, Nk=77, zero_lead=1, stats_out=False),
    _c("attn-cross-192-add-rowvec", "attention", "add_rowvec", build_attention, dim=192, heads=2, d_head=96, Nk=20, zero_lead=1,
       fold=False, stats_out=False),
    _c("attn-cross-single", "attention", "rr", build_attention, Nk=20, zero_lead=1, single=True),
    # ---- BasicTransformerBlock ----
    _c("btb-folded", "btb", "gemm[ln,geglu]", build_btb, forward=True),
    _c("btb-lnfold-off", "btb", "layernorm", build_btb, switches={"LN_FOLD": False}),
    _c("btb-unfolded-zhalf", "btb", "layernorm[out]", build_btb, switches={"LN_FOLD": False}, zero_lead=1),
    _c("btb-folded-zhalf-77", "btb", "zr", build_btb, zero_lead=1, Nk=77),
    _c("btb-disable-self-attn", "btb", "ln_rowstats gemm[] gemm[bpr,k] gemm[ln] attention gemm[res,lno] gemm[] gemm[bpr,k] gemm[ln]", build_btb, disable_self_attn=True),
    _c("btb-gelu-ff", "btb", "gemm[ln,gelu]", build_btb, glu=False),
    # ---- SpatialTransformer ----
    _c("st-conv", "st", "gemm[lno]", build_st, forward=True),
    _c("st-linear", "st", "gemm[lno]", build_st, use_linear=True),
    _c("st-depth2", "st", "gemm[ln,geglu]", build_st, depth=2),
    _c("st-96", "st", "conv_narrow", build_st, C=96, heads=8, d_head=40),
    _c("st-pair", "st", "pair_single=1", build_st, cfg_pair=True, zero_lead=1),
    _c("st-pair-copies", "st", "cat", build_st, switches={"pair_without_copies": False}, cfg_pair=True, zero_lead=1),
    _c("st-pair-linear-copies", "st", "cat cat cat", build_st, cfg_pair=True, zero_lead=1, use_linear=True),      # (pair_single_ok not asked)
    # pair_single_ok asked and False: no statistics (inner 384 does not fold), zero_lead not half the batch, no wide-tile forms
    _c("st-pair-384-no-stats", "st", "pair_single=0 cat cat", build_st, C=384, heads=4, d_head=96, cfg_pair=True, zero_lead=1),
    _c("st-pair-zero-lead-0", "st", "pair_single=0 cat cat cat", build_st, cfg_pair=True, zero_lead=0),
    _c("st-pair-gemmfuse-off", "st", "pair_single=0 cat cat cat", build_st, switches={"GEMM_FUSE": False}, cfg_pair=True, zero_lead=1),
    _c("st-pstats-off", "st", "gemm[ln,geglu] gemm[res] gemm[res]", build_st, switches={"GN_PSTATS": False}),
    _c("st-gemmfuse-off", "st", "add_rowvec", build_st, switches={"GEMM_FUSE": False}, zero_lead=1),
    # ---- miniature UNet ----
    _c("unet-plain", "unet", "groupnorm[x2,pstats]", build_unet, sep=True, forward=True),
    _c("unet-cfg-pair", "unet", "rr", build_unet, sep=False, mode="cfg_pair"),
    _c("unet-emb-table", "unet", "rpv=2^30", build_unet, sep=False, mode="emb_table"),
    _c("unet-control", "unet", "add", build_unet, sep=True, mode="control"),
    _c("unet-mix", "unet", "axpby", build_unet, sep=True, mode="mix"),
]
CASE = {c["id"]: c for c in CASES}
CLASSES = ("resblock", "resample", "attention", "btb", "st", "unet")
_BUILT = {}


def register(cases):
    """further case tables (tests/encoder_vae_refs.py) share built() / run_gpu() / the stand-in runner; CASES stays the UNet's"""
    for c in cases:
        assert CASE.setdefault(c["id"], c) is c, f"case id {c['id']} is taken"


def built(cid):
    """cases are built once per session and shared (the reference too: .ref64); nothing in them is modified afterwards"""
    b = _BUILT.get(cid)
    if b is None:
        c = CASE[cid]
        b = _BUILT[cid] = c["build"](**c["kw"])
        b.ref64 = b.ref()
    return b


# ------------------------------------------------------------------------------------------------
# path census
# ------------------------------------------------------------------------------------------------
class Census:
    """wraps the top-level `ops` calls (and torch.cat as the product modules see it) and logs, per call, the function and the flags
    that tell the forms apart.  Calls made inside another `ops` call are not logged."""

    FUNCS = ("gemm", "conv", "conv_narrow", "groupnorm", "groupnorm_table", "layernorm", "ln_rowstats", "attention", "add", "axpby",
             "add_rowvec", "activation", "cat_pair", "timestep_embedding", "to_nhwc", "to_nchw", "swin_window_attention",
             "layernorm_patch_merge", "softmax_rows")

    def __init__(self):
        self.log, self.depth = [], 0

    def token(self, name, a, k, ret, fresh=True):
        from lib.hip import ops
        f = []
        if name == "gemm":
            act = {0: None, 1: "gelu", 2: "relu", 3: "silu"}.get(k.get("act", 0), "geglu")
            for key, flag in (("ln", "ln"), ("res", "res"), ("a2", "a2")):
                if k.get(key) is not None:
                    f.append(flag)
            if act:
                f.append(act)
            f += [n for key, n in (("bias_per_row", "bpr"), ("k", "k"), ("out", "out"), ("zero_rows", "zr"), ("res_rows", "rr"),
                                   ("out_t", "ot")) if torch.is_tensor(k.get(key)) or k.get(key)]
            if ops.ln_out_arg(k.get("ln_out")) is not None:
                f.append("lno")
            if k.get("gn_out"):
                f.append("gno")
            if k.get("rowvec") is not None:
                f.append("rv")
        elif name == "conv":
            if k.get("ups"):
                f.append(f"ups={int(k['ups'])}" + (((":declined" if fresh else ":remembered") if ret is None else ":served") if k["ups"] == 2 else ""))
            if k.get("gn") is not None:
                f.append("gn+x2" if k["gn"][1] is not None else "gn")
            if k.get("gn_fuse") is not None:
                f.append("gnf=" + (("declined" if fresh else "remembered") if ret is None else "served") + (",raw" if k["gn_fuse"][4] else ""))
            if k.get("rowvec") is not None:
                f.append("rv")
                if (k.get("rows_per_rv") or 0) >= 1 << 30:
                    f.append("rpv=2^30")
            f += [n for key, n in (("res", "res"), ("out_hw", "ohw")) if k.get(key) is not None]
            if k.get("stride", 1) != 1:
                f.append("s2")
            if k.get("gn_out") and ret is not None and ops.get_gn_stats(ret) is not None:
                f.append("gno")
        elif name == "groupnorm":
            x2 = k.get("x2")
            if x2 is not None:
                f.append("x2")
            st = ops.GN_PSTATS and ops.get_gn_stats(a[0]) is not None and (x2 is None or ops.get_gn_stats(x2) is not None)
            B, C1 = a[0].shape[0], a[0].shape[-1]
            HW = a[0].numel() // (B * C1)
            if st and ops._lib().pfd_groupnorm_takes_pstats(B, C1, 0 if x2 is None else x2.shape[-1], HW, a[3]):
                f.append("pstats")
        elif name == "groupnorm_table":
            if k.get("x2") is not None:
                f.append("x2")
        elif name in ("layernorm", "add", "add_rowvec", "axpby", "softmax_rows"):
            if k.get("out") is not None:
                f.append("out")
            if k.get("ln_out") is not None:
                f.append("lno")
        return f"{name}[{','.join(f)}]" if name in ("gemm", "conv") or f else name

    def wrap(self, name, fn):
        def wrapped(*a, **k):
            from lib.hip import ops
            self.depth += 1
            known = len(ops._DECLINED)
            try:
                ret = fn(*a, **k)
            finally:
                self.depth -= 1
            if self.depth == 0:      # (a request the library declines now enters the decline memory; one answered FROM it does not)
                self.log.append(self.token(name, a, k, ret, fresh=len(ops._DECLINED) > known))
            return ret
        return wrapped

    def install(self, monkeypatch):
        from lib.hip import ops
        from lib.model_zoo import attention as AT
        for name in self.FUNCS:
            monkeypatch.setattr(ops, name, self.wrap(name, getattr(ops, name)))
        real_get = ops.get_normed

        def get_normed(t, key):
            y = real_get(t, key)
            if y is not None and self.depth == 0:
                self.log.append("normed_hit")
            return y
        monkeypatch.setattr(ops, "get_normed", get_normed)
        real_ok = AT.BasicTransformerBlock.pair_single_ok

        def pair_single_ok(blk, *a, **k):
            r = real_ok(blk, *a, **k)
            self.log.append(f"pair_single={int(bool(r))}")
            return r
        monkeypatch.setattr(AT.BasicTransformerBlock, "pair_single_ok", pair_single_ok)
        census = self

        class _Torch:
            """`torch` as lib/model_zoo/attention.py and openaimodel.py see it: torch.cat on activations is a copy the host layer chose to make"""

            def __getattr__(self, n):
                return getattr(torch, n)

            @staticmethod
            def cat(ts, *a, **k):
                if census.depth == 0:
                    census.log.append("cat")
                return torch.cat(ts, *a, **k)
        from lib.model_zoo import openaimodel as OM
        monkeypatch.setattr(AT, "torch", _Torch())
        monkeypatch.setattr(OM, "torch", _Torch())
        return self

    def rerun(self, fn):
        """run once more WITHOUT emptying the decline memory: .again holds that run's calls"""
        n = len(self.log)
        fn()
        self.log, self.again = self.log[:n], self.log[n:]

    def remembered(self):
        """what a run that starts from this run's decline memory must log: a declined phase fold is not asked again
        (Conv2d.hip), a declined fused reduction is asked and answered from the memory (ops.conv)"""
        return [t.replace("gnf=declined", "gnf=remembered") for t in self.log if "ups=2:declined" not in t]

    def line(self, cid):
        return f"{cid}: " + " ".join(self.log)

    def decisions(self):
        """[served?] of the optional-form requests, in order (what a Policy list takes)"""
        out = []
        for t in self.log:
            if ("ups=2:" in t or "gnf=" in t) and "remembered" not in t:
                out.append("served" in t)
        return out


def read_golden_paths(path):
    out = {}
    for line in open(path):
        line = line.strip()
        if line and not line.startswith("#"):
            cid, _, rest = line.partition(": ")
            out[cid] = rest.split()
    return out


def golden_decisions(tokens):
    """the library's answers to the optional-form requests that reached it, in order (requests answered from the decline memory
    reach neither the library nor a Policy)"""
    return ["served" in t for t in tokens if ("ups=2:" in t or "gnf=" in t) and "remembered" not in t]


def ref_of(b, fwd=False):
    """the fp64 formula of the case (of its .forward form where that computes something else), computed once"""
    if fwd and hasattr(b, "ref_fwd"):
        if not hasattr(b, "ref_fwd64"):
            b.ref_fwd64 = b.ref_fwd()
        return b.ref_fwd64
    return b.ref64


def run_gpu(case, census=False, fwd=False, params=False):
    """the case through the real .hip methods on the device, in a patch context of its own (switches, an empty decline memory) ->
    (output of the first run on the CPU, Census | None of a second run, whether the second run gave the same bits, whether the
    inputs are unchanged).  With census=True a THIRD run keeps the decline memory of the second: its calls are Census.again.  The
    GroupNorm statistics riding on the first run's output (or None) are Built.gn_carried; with params=True the names of the
    parameters and buffers that differ from the case's after the runs are Built.params_changed."""
    import pytest
    from lib.hip import ops
    b = built(case["id"])
    with pytest.MonkeyPatch.context() as mp:
        apply_switches(mp, case["switches"])
        mp.setattr(ops, "_DECLINED", set())
        mods, inputs = _dev(b, "cuda")
        run = b.fwd if fwd else b.run
        b.ln_carried = b.gn_carried = None          # (what the tests read afterwards belongs to THIS run)
        y0 = run(mods, inputs)
        st = ops.get_gn_stats(y0)
        b.gn_carried = None if st is None else st.detach().cpu()
        y = y0.detach().clone()
        cen, same = None, None
        if census:
            ops._DECLINED.clear()
            cen = Census().install(mp)
            same = bool(torch.equal(y, run(mods, inputs)))
            cen.rerun(lambda: run(mods, inputs))
        torch.cuda.synchronize()
        kept = all(torch.equal(v.cpu(), b.inputs[k]) for k, v in inputs.items() if torch.is_tensor(v))
        if params:      # the fp16 views of the host layer ARE the parameters of an fp16 module: none of them may be written
            b.params_changed = [f"{k}.{n}" for k, m in mods.items() for n, t in m.state_dict().items()
                                if not torch.equal(t.cpu(), b.mods[k].state_dict()[n].to(t.dtype))]
    return y.cpu(), cen, same, kept
