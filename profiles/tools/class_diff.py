#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libsxgpoa.so, kernel by kernel.

    class_diff.py OLD NEW        OLD, NEW: a build directory of objects (smoothxg_amd/csrc/build) or a linked .so

Every code object of either side is taken apart (objects: the .hip_fatbin section, unbundled; a .so: its embedded code
objects); for every kernel (symbols with a .kd descriptor) and every out-of-line device function the disassembly without
addresses and raw bytes is compared, and for every kernel the register, LDS and scratch figures of the amdhsa.kernels notes.
A literal that only differs because a pc-relative call's target moved inside the code object is counted on its own
("call offset only").  Prints added / removed / changed symbols and the totals; exit status 1 on any.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_KEYS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size",
             ".uses_dynamic_stack")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(path, tmp):
    """gfx950 ELF files of a build directory (one per object) or of a shared library (one per translation unit)"""
    out = []
    if os.path.isdir(path):
        for name in sorted(os.listdir(path)):
            if not name.endswith(".o"):
                continue
            fat = os.path.join(tmp, name + ".fat")
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, os.path.join(path, name)],
                           check=True, capture_output=True)
            co = os.path.join(tmp, name + ".co")
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                            "--targets=" + TARGET, "--output=" + co], check=True, capture_output=True)
            out.append(co)
    else:
        # a linked library: its .hip_fatbin holds the bundles of all translation units back to back
        fat = os.path.join(tmp, "so.fat")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path], check=True, capture_output=True)
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for i, s in enumerate(starts):
            piece = os.path.join(tmp, "so%d.fat" % i)
            with open(piece, "wb") as f:
                f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            co = os.path.join(tmp, "so%d.co" % i)
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + piece,
                            "--targets=" + TARGET, "--output=" + co], check=True, capture_output=True)
            out.append(co)
    return out


CALL_LIT = re.compile(r"^(\s*s_add(?:c)?_u32 s\d+, s\d+, )(0x[0-9a-f]+|-?\d+)\s*$")


def functions(co):
    """{symbol: (hash of the disassembly, hash with call-offset literals blanked)} and {kernel: notes} of one code object"""
    funcs, cur, lines = {}, None, []

    def close():
        if cur is not None:
            # (what follows a function's last instruction -- s_nop 0 and "..." -- pads the next symbol to its alignment: it moves
            #  with the sizes of the functions before it, not with this one)
            while lines and lines[-1].strip() in ("s_nop 0", "..."):
                lines.pop()
            text = "\n".join(lines)
            loose = "\n".join(CALL_LIT.sub(r"\1<rel>", l) for l in lines)
            funcs[cur] = (hashlib.sha1(text.encode()).hexdigest(), hashlib.sha1(loose.encode()).hexdigest(), len(lines))
    dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-leading-addr", "--no-show-raw-insn", co)
    for line in dis.splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            close()
            cur, lines = m.group(1), []
        elif cur is not None and line.strip():
            # (targets of branches are printed as absolute addresses in a comment / operand: keep the offset form only)
            lines.append(re.sub(r"\s*// [0-9A-Fa-f]+: .*$", "", re.sub(r"<[^>]+\+0x[0-9a-f]+>", "<L>", line)).rstrip())
    close()
    notes, cur_notes = {}, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)   # (keys of a kernel's own map; deeper ones are its arguments)
        if not m:
            continue
        if m.group(1) == "- ":
            cur_notes = {}
        if m.group(2) == ".symbol":
            notes[m.group(3).strip("'\" ")] = cur_notes
        elif m.group(2) in NOTE_KEYS:
            cur_notes[m.group(2)] = m.group(3)
    return funcs, notes


def collect(path, tmp):
    funcs, notes = {}, {}
    for co in code_objects(path, tmp):
        f, n = functions(co)
        for k, v in f.items():   # (a function local to its code object may exist in several: the 2nd is "name #2")
            i, key = 1, k
            while key in funcs:
                i += 1
                key = "%s #%d" % (k, i)
            funcs[key] = v
        notes.update(n)
    return funcs, notes


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        fa, na = collect(sys.argv[1], ta)
        fb, nb = collect(sys.argv[2], tb)
    added = sorted(set(fb) - set(fa))
    removed = sorted(set(fa) - set(fb))
    changed, call_only, notes_changed = [], [], []
    for k in sorted(set(fa) & set(fb)):
        if fa[k][0] != fb[k][0]:
            (call_only if fa[k][1] == fb[k][1] else changed).append(k)
    for k in sorted(set(na) & set(nb)):
        if na[k] != nb[k]:
            notes_changed.append(k)
    notes_added, notes_removed = sorted(set(nb) - set(na)), sorted(set(na) - set(nb))
    for title, lst in (("added", added), ("removed", removed), ("changed (instructions)", changed),
                       ("changed (call offset only)", call_only), ("changed (kernel notes: registers, LDS, scratch)", notes_changed),
                       ("kernel descriptors added", notes_added), ("kernel descriptors removed", notes_removed)):
        for k in lst:
            print("%s: %s" % (title, k))
    nk = len(set(na) & set(nb))
    print("old: %d functions, %d kernels; new: %d functions, %d kernels" % (len(fa), len(na), len(fb), len(nb)))
    print("compared: %d functions (%d instructions), %d kernel note sets" % (len(set(fa) & set(fb)), sum(fa[k][2] for k in set(fa) & set(fb)), nk))
    print("added %d, removed %d, changed %d, call-offset-only %d, notes changed %d, descriptors added %d, removed %d" %
          (len(added), len(removed), len(changed), len(call_only), len(notes_changed), len(notes_added), len(notes_removed)))
    bad = added or removed or changed or call_only or notes_changed or notes_added or notes_removed
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
