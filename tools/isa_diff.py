"""Compare kernels of two `hipcc --cuda-device-only -S` listings instruction by instruction (pure text; runs anywhere).

    python tools/isa_diff.py OLD.s NEW.s old=new [old=new ...]

old / new: regular expressions searched in the (mangled) kernel symbols of the two listings; each must match exactly one, e.g.
`attn_fwd4l_kernel=attn_fwd4_kernelILb1E`.  Comment and directive lines are dropped, `.LBB<n>_` becomes `.LBB_` and a kernel's own
symbol `<self>`; prints IDENTICAL or a unified diff per pair, and exits 1 if any pair differs."""
import difflib
import re
import sys


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


def pick(ks, pat, path):
    hits = [k for k in ks if re.search(pat, k)]
    if len(hits) != 1:
        sys.exit(f"{pat!r} matches {hits or 'nothing'} in {path}")
    return hits[0]


if __name__ == "__main__":
    old_path, new_path, pairs = sys.argv[1], sys.argv[2], [p.split("=", 1) for p in sys.argv[3:]]
    old, new, bad = kernels(old_path), kernels(new_path), 0
    for po, pn in pairs:
        ko, kn = pick(old, po, old_path), pick(new, pn, new_path)
        diff = list(difflib.unified_diff(old[ko], new[kn], ko, kn, lineterm="", n=0))
        print(f"{ko} ({len(old[ko])} lines) -> {kn} ({len(new[kn])} lines): " + ("IDENTICAL" if not diff else "DIFFERENT"))
        print("\n".join(diff), end="\n" if diff else "")
        bad += bool(diff)
    sys.exit(1 if bad else 0)
