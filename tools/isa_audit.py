#!/usr/bin/env python
"""Static audit of the generated gfx950 ISA for the two compiler behaviours that cost this code base the most
(DESIGN.md 3.2), so that they cannot come back unnoticed.  No GPU needed: hipcc -S cross-compiles.

  1. a global load written inside an `if` is emitted as branch + load + `s_waitcnt vmcnt(0)`: however many loads the
     source issues "up front", one is in flight.  Metric: `s_waitcnt vmcnt(0)` within 2 lines of a global load that
     is the ONLY load since the previous VM wait (a wait behind a batch of loads is what we want); more than two of
     those in a kernel is a finding.
  2. `__syncthreads()` next to LDS-DMA drains the DMA queue (`s_waitcnt vmcnt(0)` directly in front of `s_barrier`):
     fatal inside the K loop of a ring kernel (NBUF > 2), where a counted wait must be the last VM wait before the
     barrier.  Metric, ring kernels only: `s_barrier` preceded (within 4 lines) by a `vmcnt(0)` wait more than twice
     (prologue-free kernels have exactly the tail wait of the last K tiles and the one before the epilogue).
  3. scratch (register spills) in any kernel.

usage: isa_audit.py [file.hip ...]   (default: gemm_glds.hip gemm_conv.hip norm.hip)   -> prints one line per kernel, exit 1 on a finding
       isa_audit.py --stores [file.hip ...]   -> per kernel: registers, scratch and how many global stores carry which cache policy
"""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prompt-free-diffusion_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{REPO}/include", f"-I{CSRC}", "-Wno-unused-result",
         "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only"]
# per-kernel override of the accepted count of single loads waited for immediately (default 2: a lone operand load in
# a prologue is fine).  swin_attn.hip (relative-position-bias gathers) and step.hip (the sampler step's eps gathers) are not
# in the default file list: once per image / once per step, < 0.1 % of the loop (DESIGN.md work queue)
KNOWN = {}


# per-file flags of csrc/Makefile (register counts are compared with the library's own build)
FILE_FLAGS = {"attention3.hip": ["-fno-honor-nans"]}


def compile_asm(src):
    out = os.path.join(tempfile.gettempdir(), "pfd_isa_" + os.path.basename(src) + ".s")
    deps = [src, os.path.join(CSRC, "pfd_common.h")]
    if os.path.basename(src) == "attention3.hip":
        deps.append(os.path.join(CSRC, "attention3_kernel.h"))
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([HIPCC] + FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + [src, "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
    return out


def audit(asm_path):
    """-> {kernel: dict(loads, serialised, drained_barriers, scratch, ring)}"""
    res, name = {}, None
    last_load, window, since = -10, [], 0
    for n, line in enumerate(open(asm_path)):
        m = re.match(r"^(_Z[A-Za-z0-9_]+):", line)
        if m:
            name = m.group(1)
            res[name] = dict(loads=0, serialised=0, drained_barriers=0, scratch=0,
                             ring=bool(re.search(r"gemm160_kernelILi\dELi\dELb[01]ELi[3-9]E", name)))
            last_load, window, since = -10, [], 0
            continue
        if name is None:
            continue
        r = res[name]
        t = line.strip()
        if re.match(r"global_load_(dwordx\d|dword|ushort|ubyte|short)", t):
            r["loads"] += 1
            last_load = n
            since += 1
        elif t.startswith("s_waitcnt") and "vmcnt(" in t:
            if "vmcnt(0)" in t:
                if n - last_load <= 2 and since == 1:
                    r["serialised"] += 1
                window.append(n)
            since = 0
        elif t.startswith("s_barrier"):
            if window and n - window[-1] <= 4:
                r["drained_barriers"] += 1
        elif t.startswith("scratch_") or "buffer_store_dword" in t and "offen" in t:
            r["scratch"] += 1
        if t.startswith(".amdhsa_private_segment_fixed_size"):
            r["scratch"] += int(t.split()[-1]) > 0
    return {k: v for k, v in res.items() if "kernel" in k}


def findings(files=None):
    files = files or [os.path.join(CSRC, f) for f in ("gemm_glds.hip", "gemm_conv.hip", "norm.hip")]
    bad, rows = [], []
    for f in files:
        for k, v in sorted(audit(compile_asm(f)).items()):
            rows.append((os.path.basename(f), k, v))
            if v["serialised"] > KNOWN.get(k, 2):
                bad.append(f"{k}: {v['serialised']} of {v['loads']} global loads are waited for immediately")
            if v["scratch"]:
                bad.append(f"{k}: uses scratch")
            if v["ring"] and v["drained_barriers"] > 2:
                bad.append(f"{k}: {v['drained_barriers']} barriers behind a vmcnt(0) wait in a ring kernel")
    return bad, rows


# ---- cache policy of the global stores, with the registers and scratch of each kernel ----
STORE_FILES = ("gemm_glds.hip", "norm.hip", "attention.hip", "attention3.hip", "elementwise.hip")


def store_policies(asm_path):
    """-> {kernel: dict(plain, wt, nt, vgprs, scratch)}: global stores by cache policy (wt = write-through, the sc1 bit;
    nt = non-temporal), .amdhsa_next_free_vgpr and .amdhsa_private_segment_fixed_size"""
    res, name, meta_of = {}, None, None
    for line in open(asm_path):
        m = re.match(r"^(_Z[A-Za-z0-9_]+):", line)
        if m:
            name = m.group(1)
            res[name] = dict(plain=0, wt=0, nt=0, vgprs=0, scratch=0)
            continue
        t = line.strip()
        if t.startswith(".amdhsa_kernel "):
            meta_of = t.split()[1]
        elif t.startswith(".end_amdhsa_kernel"):
            meta_of = None
        elif meta_of in res and t.startswith(".amdhsa_next_free_vgpr"):
            res[meta_of]["vgprs"] = int(t.split()[-1])
        elif meta_of in res and t.startswith(".amdhsa_private_segment_fixed_size"):
            res[meta_of]["scratch"] = int(t.split()[-1])
        elif name is not None and t.startswith("global_store_"):
            flags = t.split(";")[0].split()
            res[name]["wt" if "sc1" in flags else "nt" if "nt" in flags else "plain"] += 1
    return {k: v for k, v in res.items() if "kernel" in k}


def store_policy_rows(files=None):
    from concurrent.futures import ThreadPoolExecutor
    files = files or [os.path.join(CSRC, f) for f in STORE_FILES]
    with ThreadPoolExecutor(len(files)) as ex:      # (the compiles run side by side: gemm_glds.hip alone takes a minute)
        asm = list(ex.map(compile_asm, files))
    return [(os.path.basename(f), k, v) for f, a in zip(files, asm) for k, v in sorted(store_policies(a).items())]


# ---- the fragment pipeline of the wave-specialised patch kernel ----
PATCH_WS = {"<2>": "conv3x3_patch_ws_kernelILi2ELi2EE", "<1>": "conv3x3_patch_ws_kernelILi1ELi2EE",
            "<0,3>": "conv3x3_patch_ws_kernelILi0ELi3EE", "<0,2>": "conv3x3_patch_ws_kernelILi0ELi2EE"}


def kernel_text(asm_path, name_part):
    """-> (instruction lines of the one kernel whose mangled name contains name_part, its .amdhsa_* directives as a dict)"""
    body, meta, name, state = [], {}, None, 0
    for line in open(asm_path):
        m = re.match(r"^(_Z[A-Za-z0-9_]+):", line)
        if m and state == 0 and name_part in m.group(1):
            name, state = m.group(1), 1
            continue
        t = line.strip()
        if state == 1:
            if t.startswith(".amdhsa_kernel") and name in t:
                state = 3
            elif t.startswith(".section") or t.startswith(".Lfunc_end"):
                state = 2
            elif t and not t.startswith(";") and not t.startswith(".") or re.match(r"^\.LBB\d+_\d+:", t):
                body.append(t.split(";")[0].strip())
        elif state == 2 and t.startswith(".amdhsa_kernel") and name in t:
            state = 3
        elif state == 3:
            m = re.match(r"^\.amdhsa_(\w+)\s+(\S+)", t)
            if m:
                meta[m.group(1)] = m.group(2)
            if t.startswith(".end_amdhsa_kernel"):
                break
    if name is None:
        raise KeyError(name_part)
    return body, meta


def mfma_loops(body):
    """backward-branch spans [label index, branch index] that hold MFMAs, innermost (shortest) first"""
    labels = {t[:-1]: i for i, t in enumerate(body) if t.endswith(":")}
    spans = []
    for i, t in enumerate(body):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", t) or re.match(r"s_branch\s+(\S+)", t)
        if m and labels.get(m.group(1), i) < i and any(x.startswith("v_mfma") for x in body[labels[m.group(1)]:i]):
            spans.append((labels[m.group(1)], i))
    return sorted(spans, key=lambda s: s[1] - s[0])


def wait_distances(seq):
    """Walk an instruction sequence: LDS reads return in order, so `s_waitcnt lgkmcnt(n)` retires all but the newest n.
    -> [(position, n, MFMAs issued since the newest read this wait retires (None: retires nothing), first wait after s_barrier)]"""
    fifo, mfmas, out, after_barrier = [], 0, [], False
    for pos, t in enumerate(seq):
        if t.startswith("ds_read") or t.startswith("ds_load"):
            fifo.append(mfmas)
        elif re.match(r"(ds_|s_load|s_buffer_load|flat_)", t):
            fifo.append(mfmas)                       # any other LGKM operation counts like a read
        elif t.startswith("v_mfma"):
            mfmas += 1
        elif t.startswith("s_barrier"):
            after_barrier = True
        elif t.startswith("s_waitcnt"):
            m = re.search(r"lgkmcnt\((\d+)\)", t)
            if not m:
                continue
            n, newest = int(m.group(1)), None
            while len(fifo) > n:
                newest = fifo.pop(0)
            out.append((pos, n, None if newest is None else mfmas - newest, after_barrier))
            after_barrier = False
    return out


def patch_pipeline_report(asm_path, name_part):
    """The consumer tap loop of one patch-kernel instantiation: resources, reads / MFMAs per loop body, and the distance
    (in MFMAs) between each LDS wait and the newest read it waits for -- in the steady state of the loop (second of two
    consecutive iterations) and along one pass of the enclosing channel-block loop (tap 0's reads, one loop body, tap 8)."""
    body, meta = kernel_text(asm_path, name_part)
    spans = [s for s in mfma_loops(body) if sum(x.startswith("v_mfma") for x in body[s[0]:s[1]]) >= 40]
    lo, hi = spans[0]
    outer = next(((a, b) for a, b in spans[1:] if a <= lo and b >= hi), None)
    loop = body[lo:hi + 1]
    rep = dict(vgprs=int(meta["next_free_vgpr"]), scratch=int(meta["private_segment_fixed_size"]),
               lds=int(meta["group_segment_fixed_size"]),
               reads=sum(t.startswith("ds_read_b128") for t in loop), other_lds=sum(t.startswith("ds_") and not t.startswith("ds_read_b128") for t in loop),
               mfmas=sum(t.startswith("v_mfma") for t in loop), barriers=sum(t.startswith("s_barrier") for t in loop),
               valu=sum(bool(re.match(r"v_(?!mfma)", t)) for t in loop))
    steady = [w for w in wait_distances(loop + loop) if w[0] >= len(loop)]
    rep["steady"] = [(n, d, first) for _, n, d, first in steady]
    rep["block"] = [(n, d, first) for _, n, d, first in wait_distances(body[outer[0]:outer[1] + 1])] if outer else []
    return rep


def patch_pipeline_main():
    asm = compile_asm(os.path.join(CSRC, "gemm_glds.hip"))
    bad = 0
    for inst, part in PATCH_WS.items():
        r = patch_pipeline_report(asm, part)
        print(f"conv3x3_patch_ws_kernel{inst}: vgprs {r['vgprs']} scratch {r['scratch']} lds {r['lds']} | tap loop: {r['reads']} ds_read_b128, "
              f"{r['mfmas']} MFMAs, {r['valu']} VALU, {r['barriers']} barrier")
        for what in ("steady", "block"):
            txt = " ".join(f"lgkmcnt({n}):{'-' if d is None else d}{'*' if first else ''}" for n, d, first in r[what])
            print(f"  {what:6s} wait:MFMAs since the read (* first after s_barrier): {txt}")
            bad += sum(1 for n, d, first in r[what] if d is not None and not first and d < 8)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--patch-pipeline"]:
        sys.exit(patch_pipeline_main())
    if sys.argv[1:2] == ["--stores"]:
        for f, k, v in store_policy_rows([os.path.abspath(a) for a in sys.argv[2:]] or None):
            print(f"{f:16s} {k} vgprs={v['vgprs']} scratch={v['scratch']} stores: plain={v['plain']} wt={v['wt']} nt={v['nt']}")
        sys.exit(0)
    bad, rows = findings([os.path.abspath(a) for a in sys.argv[1:]] or None)
    for f, k, v in rows:
        print(f"{f:14s} {k[:84]:84s} loads={v['loads']:3d} serialised={v['serialised']:2d} "
              f"vmcnt0+barrier={v['drained_barriers']:2d} scratch={v['scratch']} {'ring' if v['ring'] else ''}")
    for b in bad:
        print("FINDING:", b)
    sys.exit(1 if bad else 0)
