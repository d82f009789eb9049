"""The GroupNorm family and the split-K reduction tails, bit for bit: which cases tests/golden/norm_bits.txt holds, how their
operands are hashed and how each is launched.  The cases are the ones the fp64 suites already run -- every entry of
kernel_refs.GN_CASES through ops.groupnorm, its `table` entries through ops.groupnorm_table, every split-K entry of
kernel_refs.GEMM_CASES through ops.gemm / ops.conv (the three reduction kernels: plain, gn_out, gnf with the raw result kept
and skipped) -- built by the same seeded builders and launched by the same helpers (tests/test_norm_kernels_gpu.py,
tests/test_gemm_kernels_gpu.py).  The fixture stores a SHA-256 of each case's operands and of every output, not the tensors
(the larger cases are megabytes).  tools/record_norm_bits.py writes it on the card; tests/test_norm_bits_gpu.py holds the
library to it; tests/test_norm_bits_cpu.py checks that the operand hashes reproduce where no card is."""
import hashlib
import os

import torch

import kernel_refs as KR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_bits.txt")
SPLITK_REDUCERS = ("splitk_reduce_kernel", "splitk_reduce_gn_kernel", "splitk_reduce_gnorm_kernel")


def cases():
    """[(kind, case id)] in fixture order: gn | table | splitk"""
    out = [("gn", c["id"]) for c in KR.GN_CASES]
    out += [("table", c["id"]) for c in KR.GN_CASES if c["table"]]
    # (the unit-operand cases: the operand kinds added later run the same launches and are held to fp64 / exact bits there)
    out += [("splitk", c["id"]) for c in KR.GEMM_CASES if c["splits"] > 1 and c["operands"] == "unit"]
    return out


def _sha(tensors):
    """SHA-256 over shape, dtype and bytes of each tensor in turn (None: its name only)"""
    h = hashlib.sha256()
    for name, t in tensors:
        h.update(name.encode())
        if t is not None:
            t = t.detach().cpu().contiguous()
            h.update(f"{tuple(t.shape)}{t.dtype}".encode())
            h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def input_hash(kind, cid):
    """of everything a launch of the case reads (CPU only): the seeded operands and what the builders derive from them"""
    if kind in ("gn", "table"):
        p = KR.gn_problem(cid)
        ts = [(k, p[k]) for k in ("x1", "x2", "gamma", "beta")]
        if kind == "gn" and p["case"]["form"].startswith("pstats"):
            ts += [("st1", KR.gn_pstats(p["x1"])), ("st2", None if p["x2"] is None else KR.gn_pstats(p["x2"]))]
        return _sha(ts)
    p = KR.gemm_problem(cid)
    c = p["case"]
    o = KR.gemm_operands(p)
    ts = [(k, o[k][0] if k in o else None) for k in ("A", "A2", "W")] + [("bias", o["bias"])]
    ts += [(k, p.get(k)) for k in ("rowvec", "R", "gn_table", "gnf_gamma", "gnf_beta")]
    if c["ln"] is not None:
        assert c["ln"] != "rowstats"
        ts += [("stats", KR.gemm_ln_args(p)), ("colsum", KR.gemm_view(*o["W"]).double().sum(1).float())]
    return _sha(ts)


def run(kind, cid):
    """one launch of the case on the card -> {output name: SHA-256 of its bytes}"""
    if kind in ("gn", "table"):
        import test_norm_kernels_gpu as NG
        p = KR.gn_problem(cid)
        c = p["case"]
        d = NG._device_operands(p)
        if kind == "gn":
            return {"y": _sha([("y", NG._launch(c, d))])}
        from lib.hip import ops
        return {"table": _sha([("table", ops.groupnorm_table(d["x1"], d["gamma"], d["beta"], c["G"], c["eps"], x2=d["x2"]))])}
    import test_gemm_kernels_gpu as GG
    p = KR.gemm_problem(cid)
    c = p["case"]
    r = GG._launch(p, GG._device_operands(p))
    if "gn_out" in r:               # (the slots past 160 / (N / 32) are not written)
        r["gn_out"] = r["gn_out"][:, :, :160 // (c["N"] // 32)]
    return {k: _sha([(k, v)]) for k, v in sorted(r.items()) if v is not None}


def save(path, rows, hip_version):
    """rows: [(kind, cid, input hash, {output: hash})]"""
    with open(path, "w") as f:
        f.write(f"# tools/record_norm_bits.py, HIP {hip_version}: kind, case, SHA-256 of the operands, SHA-256 of each output\n")
        for kind, cid, hin, outs in rows:
            f.write(" ".join([kind, cid, f"in={hin}"] + [f"{k}={v}" for k, v in sorted(outs.items())]) + "\n")


def load(path=FIXTURE):
    """-> (HIP version, [(kind, cid, input hash, {output: hash})])"""
    hip, rows = None, []
    for line in open(path):
        if line.startswith("#"):
            hip = line.split("HIP ")[1].split(":")[0]
            continue
        kind, cid, *rest = line.split()
        kv = dict(t.split("=", 1) for t in rest)
        rows.append((kind, cid, kv.pop("in"), kv))
    return hip, rows
