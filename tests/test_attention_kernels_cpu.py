"""CPU: the fp64 attention references of tests/kernel_refs.py, which tests/test_attention_kernels_gpu.py holds the six kernels
behind pfd_attention_f16 against -- pinned to the oracle's attention cores (oracle/pfd_oracle.py cross_attention / vae_attn),
checked to index strided operands like dense ones, to stay far inside the GPU bound in their own arithmetic, to read no
poisoned element, and to be run on operands that tell wrong variants of the kernel from the right one."""
import os
import re

import pytest
import torch

import kernel_refs as KR
import pfd_oracle as O

ALL = KR.ATTN_CASES


class SD64(O.SD):
    """the oracle's state-dict view without its cast to fp32"""

    def __getitem__(self, k):
        return self.sd[self.prefix + k].double()

    def sub(self, p):
        return SD64(self.sd, self.prefix + p)


def _ref(p, **kw):
    B, H, Nq, Nk, D = p["dims"]
    return KR.attention_ref(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, p["scale"], **p["desc"], **kw)


def _cls(case):
    return KR.attention_kernel_class(*case[:5])


def _zero_pads(p):
    return torch.where(p["vt_valid"], p["vt"], torch.zeros((), dtype=torch.float16))


# ------------------------------------------------------------------------------------------------
# the reference is the oracle's
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ALL if c[5] == "dense" and c[4] != 512], ids=KR.attn_case_id)
def test_reference_is_the_oracles_cross_attention(case):
    """O.cross_attention with identity projections, in fp64, on the dense operands"""
    B, H, Nq, Nk, D = case[:5]
    p = KR.attention_problem(case)
    C = H * D
    eye = torch.eye(C, dtype=torch.float64)
    # (cross_attention projects k and v from ONE context: the projections select the halves of [k | v])
    sd = SD64({"to_q.weight": eye, "to_k.weight": torch.cat([eye, 0 * eye], 1), "to_v.weight": torch.cat([0 * eye, eye], 1),
               "to_out.0.weight": eye})
    x = p["q"].double().view(B, Nq, C)
    ctx = p["k"].double().view(B, Nk, C)
    v = p["vt"].view(C, B, -1)[:, :, :Nk].permute(1, 2, 0).double()
    got = O.cross_attention(sd, x, torch.cat([ctx, v], -1), H)
    e = float((got - _ref(p)).abs().max())
    print(f"[attn-kernels] reference vs oracle cross_attention {KR.attn_case_id(case)}: max abs {e:.2e}")
    assert got.dtype == torch.float64 and e <= 1e-12, e


@pytest.mark.parametrize("case", [c for c in ALL if c[4] == 512 and c[5] == "dense"], ids=KR.attn_case_id)
def test_reference_is_the_oracles_vae_attn(case):
    """O.vae_attn(x) - x with identity q / k / v / proj_out convolutions is the attention core of h = GroupNorm(x), one head of
    C = 512 over the H W tokens (self-attention: the case's query count and its Q operand set the tokens)"""
    B, H, Nq, Nk, D = case[:5]
    g = torch.Generator().manual_seed(5 + Nq)
    x = torch.randn((B, D, Nq // 8, 8), generator=g, dtype=torch.float64)
    eye = torch.eye(D, dtype=torch.float64).view(D, D, 1, 1)
    sd = SD64({"norm.weight": 1 + 0.2 * torch.randn(D, generator=g), "norm.bias": 0.1 * torch.randn(D, generator=g),
               "q.weight": eye, "k.weight": eye, "v.weight": eye, "proj_out.weight": eye})
    got = (O.vae_attn(sd, x) - x).reshape(B, D, Nq).permute(0, 2, 1)
    h = O.group_norm(sd.sub("norm."), x, 1e-6).reshape(B, D, Nq)                 # [B, C, N]: already V^T per sample
    tok = h.permute(0, 2, 1).contiguous().view(-1)
    vt = h.permute(1, 0, 2).contiguous().view(-1)
    ref = KR.attention_ref(tok, tok, vt, B, 1, Nq, Nq, D, int(D) ** -0.5, ldq=D, ldk=D, ldvt=B * Nq, q_bs=Nq * D, k_bs=Nq * D,
                           vt_bs=Nq)
    e = float((got - ref).abs().max())
    print(f"[attn-kernels] reference vs oracle vae_attn {KR.attn_case_id(case)}: max abs {e:.2e}")
    assert e <= 1e-12, e


@pytest.mark.parametrize("case", [c for c in ALL if c[5] != "dense"], ids=KR.attn_case_id)
def test_strided_reference_equals_itself_on_densified_operands(case):
    B, H, Nq, Nk, D = case[:5]
    p = KR.attention_problem(case)
    q, k, vt, desc = KR.attention_densified(p)
    for f in (KR.attention_ref, KR.attention_ref_folded):
        a = f(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, p["scale"], **p["desc"])
        b = f(q, k, vt, B, H, Nq, Nk, D, p["scale"], **desc)
        assert torch.equal(a, b), f.__name__


# ------------------------------------------------------------------------------------------------
# the cases reach what they are listed for
# ------------------------------------------------------------------------------------------------
def test_cases_cover_every_dispatch_class():
    by = {}
    for c in ALL:
        for sl in ((2, 4) if c[4] == 512 else (2,)):
            by.setdefault(KR.attention_kernel_class(*c[:5], slices=sl), []).append(c)
    assert set(by) == set(KR.ATTN_CLASSES), sorted(by, key=str)
    assert {c[3] // 64 for c in by["a3"]} >= {2, 3, 4, 5, 9}
    assert all(c[3] % 64 == 0 for c in by["a3"])
    nk8 = {c[3] for c in by["w8"]}
    assert any(n < 64 for n in nk8) and 64 in nk8 and any(n > 64 and n % 64 for n in nk8), nk8
    assert {c[5] for c in ALL} == {"dense", "fused_qk", "vt_offset", "shared_kv"}
    for c in KR.ATTN_STAIRCASE + KR.ATTN_PEAKED:
        assert c in ALL
    assert {_cls(c) for c in KR.ATTN_STAIRCASE} == set(KR.ATTN_FOLDED)
    assert {_cls(c) for c in KR.ATTN_PEAKED} == {"w4", "w8", "a3", "d80", "d96", "d160", "d512_2"}
    # the rule's own edges
    assert KR.attention_kernel_class(32, 8, 256, 128, 40) == "a3" and KR.attention_kernel_class(32, 8, 256, 64, 40) == "w4"
    assert KR.attention_kernel_class(31, 8, 256, 128, 40) == "w4" and KR.attention_kernel_class(16, 8, 1024, 128, 40) == "a3"
    assert KR.attention_kernel_class(16, 8, 1023, 148, 40) == "w4" and KR.attention_kernel_class(16, 8, 1024, 148, 40) == "w8"
    assert KR.attention_kernel_class(1, 2, 8, 8, 64) is None and KR.attention_kernel_class(1, 2, 8, 32, 512) is None
    assert KR.attention_kernel_class(1, 1, 8, 40, 512) is None


def test_restated_rule_names_the_kernel_of_every_pinned_launch():
    """the hook-free section of tests/golden/attention_dispatch.txt (the dry run of the three entry points that
    tests/test_cpu_emulation.py pins to the host code): KR.attention_kernel_class names the class of the recorded kernel on
    every line that launches, and None on every line declined with PFD_ESHAPE (-2)"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_dispatch.txt")).read()
    section = text.split("# hooks: ")[1].splitlines()
    assert section[0] == "none" and len(section) > 300
    seen = set()
    for line in section[1:]:
        m = re.match(r"^(plain|kbias|rbias) (\d+) (\d+) (\d+) (\d+) (\d+)(.*) -> (-?\d+)(?: \| (.+) grid \d+ block \d+)?$", line)
        assert m, line
        rc, kernel = int(m.group(8)), m.group(9)
        assert (rc == 0) == (kernel is not None), line
        if rc == -1:                                 # PFD_EINVAL: the descriptor checks in front of the rule
            continue
        sl = re.search(r"slices=(\d+)", m.group(7))
        got = KR.attention_kernel_class(*map(int, m.group(2, 3, 4, 5, 6)), slices=int(sl.group(1)) if sl else 2,
                                        operand=None if m.group(1) == "plain" else m.group(1))
        assert got == (KR.ATTN_KERNEL_CLASS[kernel] if kernel else None), (line, got)
        seen.add((m.group(1), got))
    assert {c for api, c in seen if api == "plain"} == set(KR.ATTN_CLASSES) | {None}
    assert {c for api, c in seen if api == "kbias"} == {"w4", "w8", "d80", "d160", None}
    assert {c for api, c in seen if api == "rbias"} == {"w4", "d80", "d160", None}


# ------------------------------------------------------------------------------------------------
# the reference's own arithmetic, and the poison
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,case", [(None, c) for c in ALL] + [("staircase", c) for c in KR.ATTN_STAIRCASE]
                         + [("peaked", c) for c in KR.ATTN_PEAKED],
                         ids=lambda v: v if isinstance(v, str) else "" if v is None else KR.attn_case_id(v))
def test_reference_is_finite_and_fp32_stays_within_an_eighth_of_the_bound(variant, case):
    """no poisoned element reaches either reference; the same formula in fp32 (CPU) is within 1/8 of the GPU bound of the
    fp64 one, so the bound is not spent on the reference"""
    p = KR.attention_problem(case, variant)
    B, H, Nq, Nk, D = p["dims"]
    ref = _ref(p)
    assert bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(KR.attention_ref_folded(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, p["scale"], **p["desc"])).all())
    e32 = float((_ref(p, dtype=torch.float32).double() - ref).abs().max())
    bound = KR.attention_bound(Nk, p["vmax"])
    print(f"[attn-kernels] fp32 formula vs fp64 {KR.attn_case_id(case)} {variant or ''}: {e32:.2e} = {e32 / bound:.4f} of the bound")
    assert e32 <= bound / 8, (e32, bound)


# ------------------------------------------------------------------------------------------------
# the operands discriminate
# ------------------------------------------------------------------------------------------------
def _applies(mutant, case):
    """whether the slip of `mutant` can show in `case` at all"""
    B, H, Nq, Nk, D, layout, spike = case
    if mutant == "last_key_dropped":
        return Nk > 1
    if mutant == "masked_keys_score_zero":      # the kernels that mask a ragged 64-key tile (d = 512 takes whole 32-key tiles only)
        return Nk % 64 != 0 and D != 512
    if mutant in ("vt_batch0", "k_batch0"):
        return B > 1 and layout != "shared_kv"
    return Nk % 8 != 0                            # v_pad_column_read


# A condition on the inputs, computed from the references alone.  The cases that separated each mutant when this was written
# (the first of each class in list order; excess over the bound):
#   last_key_dropped        w4 q77k64 fused 153 x, w8 q1024k148 vt_offset 24 x, a3 q256k128 23 x, d80 q64k64 344 x,
#                           d96 q144k256 223 x, d160 q64k148 85 x, d512 q128k32 402 x
#   masked_keys_score_zero  w4 q300k148 12 x, w8 q1024k8 36 x, d80 q150k148 11 x, d96 q148k148 10 x, d160 q64k148 9 x
#   vt_batch0 / k_batch0    w4 q77k64 fused 540 / 425 x, w8 q1024k148 vt_offset 48 / 49 x, a3 q256k128 45 / 38 x,
#                           d80 q64k64 552 / 572 x, d160 q64k148 425 / 378 x, d512 B2 q128k512 fused 531 / 400 x
#   v_pad_column_read       w4 q300k148 650 x, w8 q1024k148 vt_offset 48 x, d80 / d96 / d160 at 148 keys 524 / 564 / 476 x
# (the folded classes carry the A term in their bound, hence their smaller figures)
@pytest.mark.parametrize("mutant", KR.ATTN_MUTANTS)
def test_operands_tell_wrong_variants_apart(mutant):
    """each wrong variant of the reference exceeds the GPU bound (with the folded term where the class has it) at least 4
    times on some element of at least one case of every class it applies to"""
    classes = {}
    for c in ALL:
        if _applies(mutant, c):
            classes.setdefault(_cls(c).split("_")[0], []).append(c)
    assert classes, mutant
    for cls, cases in classes.items():
        best = (0.0, None)
        for c in cases:
            p = KR.attention_problem(c)
            B, H, Nq, Nk, D = p["dims"]
            A = KR.attention_fold_amplitude(p["q"], p["k"], B, H, Nq, Nk, D, p["scale"], **p["desc"]) if cls in KR.ATTN_FOLDED else 0.0
            vt = _zero_pads(p) if mutant == "v_pad_column_read" else p["vt"]      # (the numbers, not the NaNs, must differ)
            wrong = KR.attention_ref(p["q"], p["k"], vt, B, H, Nq, Nk, D, p["scale"], **p["desc"], mutant=mutant)
            r = float((wrong - _ref(p)).abs().max()) / KR.attention_bound(Nk, p["vmax"], A)
            if r > best[0]:
                best = (r, c)
            if r >= 4:
                break
        print(f"[attn-kernels] mutant {mutant}, class {cls}: {best[0]:.1f} x the bound on {KR.attn_case_id(best[1]) if best[1] else None}")
        assert best[0] >= 4, (mutant, cls, best)


def test_variants_only_differ_where_they_apply():
    """a mutant is the reference itself where its slip cannot show"""
    for case in ((1, 1, 33, 1, 40, "dense", 0), (1, 8, 144, 256, 96, "dense", 0), (3, 2, 64, 148, 40, "shared_kv", 0)):
        p = KR.attention_problem(case)
        for m in KR.ATTN_MUTANTS:
            if not _applies(m, case):
                assert torch.equal(_ref(p, mutant=m), _ref(p)), (case, m)


def test_staircase_operands_rise_five_per_tile():
    """the tile maxima of the folded scores of the staircase operands: + 5 (within 0.15) per 64-key tile for every query"""
    for case in KR.ATTN_STAIRCASE:
        p = KR.attention_problem(case, "staircase")
        B, H, Nq, Nk, D = p["dims"]
        d = p["desc"]
        Q, K, _ = KR._attn_views(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, d["ldq"], d["ldk"], d["ldvt"], d["q_bs"], d["k_bs"],
                                 d["vt_bs"], d["q_off"], d["k_off"], d["vt_off"])
        s = (Q[0].float() * torch.tensor(p["scale"] * KR.LOG2E)).half().double() @ K[0].double().transpose(-1, -2)     # [H, Nq, Nk]
        nt = -(-Nk // 64)
        tops = torch.stack([s[..., 64 * t:64 * t + 64].amax(-1) for t in range(nt)], -1)
        rise = tops[..., 1:] - tops[..., :-1]
        assert float((rise - 5).abs().max()) <= 0.15, (float(rise.min()), float(rise.max()))
        assert float(tops[..., 0].abs().max()) <= 0.15
