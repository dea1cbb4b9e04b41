"""Compare kernels of two `hipcc --cuda-device-only -S` listings instruction by instruction (pure text; runs anywhere).

    python tools/isa_diff.py OLD.s NEW.s old=new [old=new ...]

old / new: regular expressions searched in the (mangled) kernel symbols of the two listings; each must match exactly one, e.g.
`attn_fwd4l_kernel=attn_fwd4_kernelILb1E`.  Comment and directive lines are dropped, `.LBB<n>_` becomes `.LBB_` and a kernel's own
symbol `<self>`.  Per pair it prints
  - the instruction-line counts and IDENTICAL or DIFFERENT,
  - whether the span from the first to the last v_mfma line is the same (`mfma span: same | DIFFERENT | none`),
  - the resource lines of the kernel's metadata record (registers, spills, LDS, scratch): one `resources: same` line, or every
    value that moved as `old -> new`,
  - for a DIFFERENT pair the unified diff,
and exits 1 if the instruction lines of any pair differ, as before."""
import difflib
import re
import sys

RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size")


def kernels(path):
    """{symbol: [instruction and label lines]} of every function in a listing"""
    out, cur = {}, None
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
        if m and not m.group(1).startswith("."):
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.strip() and (not line.strip().startswith(".") or line.startswith(".LBB")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return {k: [l.replace(k, "<self>") for l in v] for k, v in out.items()}


def resources(path):
    """{symbol: {resource key: value}} from the kernel records of the listing's amdgpu_metadata"""
    out, rec = {}, None
    for line in open(path):
        if line.startswith("  - ."):          # a new kernel record (argument records sit deeper)
            rec = {}
        m = re.match(r"^  [ -] (\.\w+):\s*(\S+)\s*$", line)
        if rec is None or not m:
            continue
        if m.group(1) == ".name":
            out[m.group(2)] = rec
        elif m.group(1) in RESOURCES:
            rec[m.group(1)] = m.group(2)
    return out


def mfma_span(lines):
    at = [i for i, l in enumerate(lines) if l.lstrip().startswith("v_mfma")]
    return lines[at[0]:at[-1] + 1] if at else None


def pick(ks, pat, path):
    hits = [k for k in ks if re.search(pat, k)]
    if len(hits) != 1:
        sys.exit(f"{pat!r} matches {hits or 'nothing'} in {path}")
    return hits[0]


if __name__ == "__main__":
    old_path, new_path, pairs = sys.argv[1], sys.argv[2], [p.split("=", 1) for p in sys.argv[3:]]
    old, new, bad = kernels(old_path), kernels(new_path), 0
    old_res, new_res = resources(old_path), resources(new_path)
    for po, pn in pairs:
        ko, kn = pick(old, po, old_path), pick(new, pn, new_path)
        diff = list(difflib.unified_diff(old[ko], new[kn], ko, kn, lineterm="", n=0))
        print(f"{ko} ({len(old[ko])} lines) -> {kn} ({len(new[kn])} lines): " + ("IDENTICAL" if not diff else "DIFFERENT"))
        so, sn = mfma_span(old[ko]), mfma_span(new[kn])
        print("  mfma span: " + ("none" if so is None and sn is None else "same" if so == sn else "DIFFERENT"))
        ro, rn = old_res.get(ko, {}), new_res.get(kn, {})
        moved = [f"{k} {ro.get(k, '?')} -> {rn.get(k, '?')}" for k in RESOURCES if ro.get(k) != rn.get(k)]
        print("  resources: " + ("same  " + " ".join(f"{k[1:]}={ro[k]}" for k in RESOURCES if k in ro) if not moved else "; ".join(moved)))
        print("\n".join(diff), end="\n" if diff else "")
        bad += bool(diff)
    sys.exit(1 if bad else 0)
