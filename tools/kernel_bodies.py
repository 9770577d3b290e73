"""Compare the gfx950 machine code of the library's kernels between two source trees, kernel by kernel, without a GPU.

  python tools/kernel_bodies.py emit <csrc dir> <out dir>     compile every .hip of the Makefile's SRCS to device assembly (-S)
  python tools/kernel_bodies.py compare <old dir> <new dir>   hash each kernel body and report

A kernel body is the text from the kernel's label to s_endpgm with comments stripped and the .LBB<n>_ labels renumbered, so a
kernel whose mangled name changed (a template parameter dropped) still matches by body.  Matching is pooled over the .s files of a
tree, so a kernel that moved to another translation unit matches too.  compare prints, per translation unit, the kernel counts, the
kernels whose body is in no file of the new tree, and every kernel of the new tree whose body is in no file of the old one (there should
be none when only dispatch code changed or kernels moved); exit status 1 if there is one."""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def emit(csrc, out):
    mk = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS \?= (.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    srcs = re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    os.makedirs(out, exist_ok=True)

    def one(s):
        subprocess.run(['/opt/rocm/bin/hipcc', *flags, '--cuda-device-only', '-S', os.path.join(csrc, s), '-o',
                        os.path.join(out, s.replace('.hip', '.s'))], check=True)
    with ThreadPoolExecutor(min(8, os.cpu_count() or 2)) as ex:
        list(ex.map(one, srcs))


def bodies(path):
    """{kernel name: sha1 of its normalised body} of one .s file"""
    txt = open(path).read()
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', txt, re.M))
    out, name, buf = {}, None, []
    for line in txt.split('\n'):
        m = re.match(r'^(\S+):', line)
        if m and m.group(1) in kernels and name is None:
            name, buf = m.group(1), []
            continue
        if name is None:
            continue
        line = re.sub(r'\s*(;|//).*$', '', line).strip()
        if not line:
            continue
        buf.append(line)
        if line == 's_endpgm':
            body = '\n'.join(buf)
            ids = {}
            body = re.sub(r'\.LBB\d+_', lambda q: ids.setdefault(q.group(0), '.L%d_' % len(ids)), body)
            out[name] = hashlib.sha1(body.encode()).hexdigest()
            name = None
    return out


def demangle(names):
    if not names:
        return []
    return subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')[:len(names)]


def compare(old, new):
    """Matching is pooled: a body of the new tree counts as unchanged when it occurs in ANY .s file of the old tree (and a kernel of the
    old tree as gone when its body occurs in none of the new ones), so a kernel that moved to another translation unit still matches.
    The per-file lines say where the kernels are; the verdict is the pooled total."""
    def tree(d):
        return {f: bodies(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.s')}
    a_all, b_all = tree(old), tree(new)
    old_hashes = {h for a in a_all.values() for h in a.values()}
    new_hashes = {h for b in b_all.values() for h in b.values()}
    bad = lost = 0
    for f in sorted(set(a_all) | set(b_all)):
        a, b = a_all.get(f, {}), b_all.get(f, {})
        changed = [k for k, h in b.items() if h not in old_hashes]
        gone = [k for k, h in a.items() if h not in new_hashes]
        moved_out = sum(1 for h in a.values() if h in new_hashes and h not in set(b.values()))
        moved_in = sum(1 for h in b.values() if h in old_hashes and h not in set(a.values()))
        print('%-22s %3d -> %3d kernels, %d gone, %d with a body not in the old build%s' % (
            f, len(a), len(b), len(gone), len(changed), ' (%d moved out, %d moved in)' % (moved_out, moved_in) if moved_out or moved_in else ''))
        for d in demangle(gone):
            print('    gone     ' + d)
        for d in demangle(changed):
            print('    CHANGED  ' + d)
        bad += len(changed)
        lost += len(gone)
    tot = [sum(map(len, a_all.values())), sum(map(len, b_all.values()))]
    print('total %d -> %d kernels, %d gone; %s' % (tot[0], tot[1], lost, 'every surviving body occurs in the old build' if not bad else
                                                   '%d bodies differ' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == 'emit':
        emit(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
