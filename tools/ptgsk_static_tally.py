"""Static tallies of the pt_gs_k run-kernel instances from the compiler's assembly.

usage: python tools/ptgsk_static_tally.py [extra hipcc flags ...]
Compiles shyft_amd/csrc/kernels/ptgsk.hip for gfx950 with the Makefile's PTGSK flags plus the extra ones, device
side only, and prints for every ptgsk_run_kernel instance: SGPR / VGPR spill counts, scratch bytes per lane, LDS
bytes, and the v_readlane / v_writelane / scratch instructions inside the outermost loop (the step loop: from the
first label a backward branch targets to the last backward branch). Needs no GPU."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shyft_amd", "csrc")


def make_var(name):
    out = subprocess.run(["make", "-s", "-C", CSRC, "--eval", f"pv:\n\t@echo $({name})", "pv"], capture_output=True,
                         text=True, check=True).stdout
    return out.split()


def loop_span(body):
    pos = {}
    for k, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            pos[m.group(1)] = k
    lo, hi = None, None
    for k, ln in enumerate(body):
        m = re.match(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
        if m and pos.get(m.group(1), k + 1) <= k:
            lo = pos[m.group(1)] if lo is None else min(lo, pos[m.group(1)])
            hi = k
    return (lo, hi) if lo is not None else (0, 0)


def main():
    flags = make_var("HIPFLAGS") + make_var("PTGSK_FLAGS") + sys.argv[1:]
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "ptgsk.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags +
                       ["--cuda-device-only", "-S", "-o", asm, os.path.join(CSRC, "kernels", "ptgsk.hip")], check=True)
        text = open(asm).read()
    lines = text.splitlines()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in
                                   ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                    "group_segment_fixed_size", "sgpr_count", "vgpr_count")}
    print(f"{'instance':52s} sgpr_sp vgpr_sp scratchB   LDS  sgpr vgpr | loop: readlane writelane scratch")
    for name, m in sorted(meta.items()):
        if "ptgsk_run_kernel" not in name:
            continue
        a = next(k for k, ln in enumerate(lines) if ln.startswith(name + ":"))
        b = next(k for k in range(a, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body = lines[a:b]
        lo, hi = loop_span(body)
        loop = body[lo:hi + 1]
        cnt = lambda pat: sum(1 for ln in loop if re.match(rf"^\s+{pat}", ln))
        demangled = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        short = re.sub(r".*ptgsk_run_kernel(<.*>).*", r"\1", demangled).replace("(bool)", "").replace(" ", "")
        print(f"{short:52s} {m['sgpr_spill_count']:7d} {m['vgpr_spill_count']:7d} {m['private_segment_fixed_size']:8d} "
              f"{m['group_segment_fixed_size']:5d} {m['sgpr_count']:5d} {m['vgpr_count']:4d} |       "
              f"{cnt('v_readlane'):8d} {cnt('v_writelane'):9d} {cnt('scratch_'):7d}")


if __name__ == "__main__":
    main()
