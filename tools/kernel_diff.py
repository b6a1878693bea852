"""Per-kernel comparison of the gfx950 code objects of two builds of the library (no GPU needed).

    python tools/kernel_diff.py [--rename OLD=NEW] PARENT_OBJ_DIR NEW_OBJ_DIR [unit ...]

The directories hold the object files of `make -C mpyc_amd/csrc` (build/ffgpu/*.o).  For every translation unit the
device code is taken out of .hip_fatbin (llvm-objcopy, clang-offload-bundler) and compared kernel by kernel:
disassembly (llvm-objdump -d, comments and addresses dropped) and the metadata of the notes (registers, LDS, scratch,
kernarg size).  Prints kernels before -> after, the kernels removed and added, those whose code or metadata changed (with
the metadata and the instruction count before -> after), and apart from them, not counted as changed:
  * those whose only difference is the PC-relative distance to a callee that was not inlined;
  * those with the same instructions in another order: the sorted instruction lines and all metadata are equal.
--rename OLD=NEW: a type that appears in the kernels' mangled names was renamed and nothing else; OLD is replaced by NEW in
the parent's names (both as mangled, with their length prefix: 6CxRows=9ShareRows) so that the kernels pair up by the rest of
the name instead of showing as removed and added (profiles/r20_share_rows.md).
A refactor of the host side must show 0 added and 0 changed (profiles/r10_host_layer.md); a refactor of the kernel source may
show changed kernels only among the templates it touched (profiles/r11_streaming_shape.md)."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
META = r'\.(vgpr_count|sgpr_count|agpr_count|group_segment_fixed_size|private_segment_fixed_size|kernarg_segment_size|' \
       r'max_flat_workgroup_size|wavefront_size|uses_dynamic_stack|vgpr_spill_count|sgpr_spill_count):'


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def extract(obj, tmp, tag):
    fb, co = os.path.join(tmp, tag + '.fatbin'), os.path.join(tmp, tag + '.co')
    run(os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', obj, fb)
    if not os.path.exists(fb) or os.path.getsize(fb) == 0:
        return None
    run(os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o',
        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fb, '--output=' + co)
    return co


def digest(buf):
    # objdump's `...` at the END of a kernel is the zero padding up to the next one (a section's last kernel has none): not
    # code.  Inside a body the mark stands for a run of zeros that is part of the kernel, and stays.
    while buf and buf[-1] == '...':
        buf = buf[:-1]
    """(exact, position-free, order-free, instructions): the second with the displacement of `s_getpc_b64; s_add_u32 lo,
    lo, DISP` masked -- the distance to a callee that was not inlined moves when code between the two is removed, the
    instructions do not; the third over the sorted lines of the second"""
    free = [re.sub(r'0x[0-9a-f]+$', 'DISP', l) if l.startswith('s_add_u32') and i and buf[i - 1].startswith('s_getpc_b64') else l
            for i, l in enumerate(buf)]
    return tuple(hashlib.sha256('\n'.join(b).encode()).hexdigest() for b in (buf, free, sorted(free))) + (sum(1 for l in buf if l),)


def code(co):
    out, name, buf = {}, None, []
    for line in run(os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', co).splitlines():
        m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:$', line)
        if m:
            if name:
                out[name] = digest(buf)
            name, buf = m.group(1), []
        elif name:
            text = re.sub(r'//.*$', '', line).strip()
            if text:
                buf.append(text)
    if name:
        out[name] = digest(buf)
    return out


def metadata(co):
    txt = run(os.path.join(LLVM, 'llvm-readelf'), '--notes', co)
    out = {}
    for ent in re.split(r'\n  - ', txt[txt.find('amdhsa.kernels:'):])[1:]:
        m = re.search(r'\.name:\s+(\S+)', ent)
        if m:
            out[m.group(1)] = tuple(sorted(l.strip() for l in ent.splitlines() if re.search(META, l)))
    return out


def main():
    args, old, new = sys.argv[1:], None, None
    if args[0] == '--rename':
        old, new = args[1].split('=')
        args = args[2:]
    renamed = lambda d: {(k.replace(old, new) if old else k): v for k, v in d.items()}
    pd, nd = args[0], args[1]
    units = args[2:] or sorted(os.path.basename(f)[:-2] for f in glob.glob(os.path.join(pd, '*.o')))
    total, bad = [0, 0], 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            a, b = extract(os.path.join(pd, u + '.o'), tmp, 'a_' + u), extract(os.path.join(nd, u + '.o'), tmp, 'b_' + u)
            if a is None or b is None:
                print(f'{u}: no device code')
                continue
            ca, cb, ma, mb = renamed(code(a)), code(b), renamed(metadata(a)), metadata(b)
            removed, added = sorted(set(ma) - set(mb)), sorted(set(mb) - set(ma))
            differ = [k for k in ca if k in cb and ca[k][1] != cb[k][1]]
            reordered = [k for k in differ if ca[k][2] == cb[k][2] and ma.get(k) == mb.get(k)]
            changed = [k for k in differ if k not in reordered]
            moved = [k for k in ca if k in cb and ca[k][1] == cb[k][1] and ca[k][0] != cb[k][0]]
            mchanged = [k for k in ma if k in mb and ma[k] != mb[k]]
            total[0] += len(ma)
            total[1] += len(mb)
            bad += bool(added or changed or mchanged)
            print(f'{u}: kernels {len(ma)} -> {len(mb)}; removed {len(removed)}, added {len(added)}, '
                  f'code changed {len(changed)}, metadata changed {len(mchanged)}, same code at another distance from a callee {len(moved)}, '
                  f'same instructions in another order {len(reordered)}')
            for tag, names in (('-', removed), ('+', added), ('~', changed), ('m', mchanged), ('d', moved), ('o', reordered)):
                for k in names:
                    print('   ', tag, k)
                    if tag in '~m':
                        print('        instructions', ca[k][3], '->', cb[k][3],
                              *(f'{x.split(":")[0]} {x.split()[-1]} -> {y.split()[-1]}' for x, y in zip(ma.get(k, ()), mb.get(k, ())) if x != y))
    print(f'total kernels {total[0]} -> {total[1]}; units with added or changed kernels: {bad}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
