"""Compare the compiled kernels of two librr builds, kernel symbol by kernel symbol.

A refactor that only moves source around must leave every kernel as it was.  For each
csrc/build/rr_*.o of both builds (rr_build.o, the source digest, aside) this takes the gfx950
code object apart and compares, per function symbol:
  * the disassembled instruction text (addresses and encodings dropped: a kernel may move
    inside its object);
  * the kernel metadata .vgpr_count, .sgpr_count, .group_segment_fixed_size and
    .private_segment_fixed_size (llvm-readelf --notes).
One line per kernel; exit 1 on a difference or on a kernel that only one side has.

    python3 tools/isa_diff.py OLD_BUILD NEW_BUILD
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dma_audit  # noqa: E402

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def functions(lines):
    """llvm-objdump -d lines -> {symbol: [instruction text]}"""
    out, body = {}, None
    for ln in lines:
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            body = out.setdefault(m.group(1), [])
            continue
        ins = ln.split("//")[0].strip()
        if body is not None and ins:
            body.append(re.sub(r"\s+", " ", ins))
    return out


def metadata(lines):
    """llvm-readelf --notes lines -> {kernel: {field: value}} for the fields of META"""
    out, cur = {}, None

    def close():
        if cur and ".name" in cur:
            out[cur[".name"]] = {k: cur.get(k) for k in META}

    for ln in lines:
        if re.match(r"^  - \.", ln):  # next entry of amdhsa.kernels (its .args entries sit deeper)
            close()
            cur = {}
        m = re.match(r"^  (?:- |  )(\.\w+):\s+(\S+)\s*$", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    close()
    return out


def compare(old_fn, old_md, new_fn, new_md):
    """-> [(symbol, verdict)], verdict "same" or what differs"""
    rows = []
    for k in sorted(set(old_fn) | set(new_fn) | set(old_md) | set(new_md)):
        if (k in old_fn or k in old_md) != (k in new_fn or k in new_md):
            rows.append((k, "only in the %s build" % ("old" if (k in old_fn or k in old_md) else "new")))
            continue
        what = []
        a, b = old_fn.get(k, []), new_fn.get(k, [])
        if a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            what.append("instruction %d of %d / %d: %r -> %r" % (i, len(a), len(b), a[i] if i < len(a) else None,
                                                                 b[i] if i < len(b) else None))
        ma, mb = old_md.get(k), new_md.get(k)
        if (ma is None) != (mb is None):
            what.append("kernel metadata on one side only")
        elif ma:
            what += ["%s %s -> %s" % (f, ma[f], mb[f]) for f in META if ma[f] != mb[f]]
        rows.append((k, "; ".join(what) if what else "same"))
    return rows


def load(obj, tmp):
    co = dma_audit.code_object(obj, tmp)
    if co is None:
        return {}, {}
    notes = subprocess.run([dma_audit.LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    return functions(dma_audit.disassemble(obj, tmp)), metadata(notes.splitlines())


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = sys.argv[1:]

    def names(d):
        return {os.path.basename(o) for o in glob.glob(os.path.join(d, "rr_*.o"))} - {"rr_build.o"}

    nkern = nbad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(names(old) | names(new)):
            if o not in names(old) or o not in names(new):
                print("%s: only in the %s build" % (o, "old" if o in names(old) else "new"))
                nbad += 1
                continue
            rows = compare(*load(os.path.join(old, o), tmp), *load(os.path.join(new, o), tmp))
            for k, verdict in rows:
                print("%s %s: %s" % (o, k, verdict))
            nkern += len(rows)
            nbad += sum(v != "same" for _, v in rows)
    print("kernels compared: %d, different: %d" % (nkern, nbad))
    sys.exit(1 if nbad else 0)


if __name__ == "__main__":
    main()
