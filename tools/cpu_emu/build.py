#!/usr/bin/env python
"""Build the CPU emulation of csrc/gemm_glds.hip, csrc/norm.hip, csrc/attention.hip, csrc/image.hip, csrc/canny.hip, csrc/latent.hip, csrc/inpaint.hip, csrc/step.hip, csrc/control.hip, csrc/guidance.hip and csrc/elementwise.hip (tools/cpu_emu/emu_*.cpp): write
<file>_emu.inc = the kernel file with its gfx950 inline-asm statements replaced by their C meaning, then compile the
drivers for the host with clang++.
(emu_attn drives pfd_attention_f16 and, with --kbias, pfd_attention_kbias_f16: the LDS-DMA load of the key logits is the shim's
__builtin_amdgcn_global_load_lds, the opaque register pins of its KBIAS builds fall under the first substitution below.)
usage: [EMU_DEFINES="-DPFD_FAST_PROLOGUE ..."] build.py [outdir]   (default /tmp/pfd_cpu_emu)  -> <outdir>/emu_gemm, <outdir>/emu_norm, <outdir>/emu_attn, <outdir>/emu_image, <outdir>/emu_canny, <outdir>/emu_latent, <outdir>/emu_inpaint, <outdir>/emu_step, <outdir>/emu_control, <outdir>/emu_guidance, <outdir>/emu_elementwise"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
CSRC = os.environ.get("EMU_CSRC") or os.path.join(REPO, "prompt-free-diffusion_amd", "csrc")   # EMU_CSRC: the kernel files of another checkout
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")

SUBST = [
    # a copy lands when it is issued; the wait is still a lockstep point of the wave (see hip_runtime.h)
    (r'asm volatile\("s_waitcnt lgkmcnt\(0\)" ::: "memory"\);', 'emu::wave_sync();'),
    # register pins / opaque values
    (r'asm volatile\("" : "\+v"\(([^;]*?)\)\);', '((void)0);'),
    (r'asm volatile\("" : "\+v"\(r\), "\+v"\(ch\)\);', '((void)0);'),
    (r'asm volatile\("" : "\+s"\(k\)::"memory"\);', '((void)0);'),
    (r'(?s)asm volatile\("" ::"s"\(p\.tiles_m\).*?\);', '((void)0);'),   # the argument-load batch at kernel entry (PFD_ARG_BATCH_*)
    (r'asm volatile\("" ::"v"\(t\)\);', '((void)0);'),
    # the register move that keeps an f16 rounding from being elided (elementwise.hip, round_f16)
    (r'asm volatile\("v_mov_b32 %0, %1" : "=v"\(b2\) : "v"\(bits\)\);', 'b2 = bits;'),
    # the opaque 16-byte LDS store of the GroupNorm prologue
    (r'asm volatile\("ds_write_b128 %0, %1" ::"v"\(addr\), "v"\(d\) : "memory"\);', 'memcpy(lds_dst, &d, 16); (void)addr;'),
]


def preprocess(name, out, required=True, ext=".hip", outname=None):
    src = open(os.path.join(CSRC, name + ext)).read()
    for pat, rep in SUBST:
        src, n = re.subn(pat, rep, src)
    # (the PFD_ARG_BATCH_* macro bodies are compiled only outside the emulation: #if ... && !defined(PFD_CPU_EMU))
    left = [l for l in src.splitlines() if "asm volatile" in l and 'asm volatile("" :::' not in l and '"s"((p).tiles_m)' not in l]
    if left:
        sys.exit(f"build.py: inline asm in {name}.hip the emulation does not translate:\n" + "\n".join(left))
    with open(os.path.join(out, outname or name + "_emu.inc"), "w") as f:
        f.write(src)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/pfd_cpu_emu"
    os.makedirs(out, exist_ok=True)
    procs = []
    only = os.environ.get("EMU_ONLY", "").split()     # e.g. EMU_ONLY=emu_gemm: just that driver
    for name, driver in (("gemm_glds", "emu_gemm"), ("norm", "emu_norm"), ("attention", "emu_attn"), ("image", "emu_image"),
                         ("canny", "emu_canny"), ("latent", "emu_latent"), ("inpaint", "emu_inpaint"), ("step", "emu_step"),
                         ("elementwise", "emu_elementwise"), ("control", "emu_control"), ("guidance", "emu_guidance")):
        if only and driver not in only:
            continue
        preprocess(name, out)
        if name == "attention":     # the kernel text attention.hip includes twice (with and without the key logits), under its own name
            preprocess("attention2_kernel", out, ext=".inc", outname="attention2_kernel.inc")
        if name == "control" and "emu_elementwise" not in [os.path.basename(e) for e, _, _ in procs]:
            # its driver also runs pfd_add_f16 (elementwise.hip), the launch the scaled add stands in for; emu_elementwise's
            # compile, if it runs, is reading that file already
            preprocess("elementwise", out)
        if name == "guidance" and "emu_step" not in [os.path.basename(e) for e, _, _ in procs]:
            # its driver also runs pfd_cfg_step_mul (step.hip); emu_step's compile, if it runs, is reading that file already
            preprocess("step", out)
        exe = os.path.join(out, driver)
        cmd = [CXX, "-std=c++17", os.environ.get("EMU_OPT", "-O0"), "-pthread", "-w", f"-I{HERE}", f"-I{out}", f"-I{REPO}/include", f"-I{CSRC}",
               os.path.join(HERE, driver + ".cpp"), "-o", exe] + os.environ.get("EMU_DEFINES", "").split()
        procs.append((exe, cmd, subprocess.Popen(cmd)))     # the drivers compile side by side
    for exe, cmd, p in procs:
        if p.wait() != 0:
            sys.exit("build.py: " + " ".join(cmd) + " failed")
        print(exe)


if __name__ == "__main__":
    main()
