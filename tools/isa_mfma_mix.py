"""Instruction mix of the MFMA loops of the matrix-core convolution kernels, from the gfx950 assembly.

usage: python tools/isa_mfma_mix.py [name filter]        (default filter: k_conv_bwd_data_v2)

Compiles vae_conv_v2.hip (and vae_conv_tiled.hip for the first engine's kernels) with `--cuda-device-only -S` into a temporary
directory and, per kernel whose mangled name contains the filter, reports every basic block with at least 16 MFMAs: MFMAs,
other vector (VALU) instructions (in the whole block, and in the k-loop proper: first LDS operand read to last MFMA), LDS reads
and `s_waitcnt` -- and the non-MFMA VALU instructions per MFMA, the quantity the cost model of DESIGN §4.3 charges (cycles per SIMD ~ 32 x MFMAs + 4 x every other vector instruction of the SIMD)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vae-gp-ode_amd', 'csrc')
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-Wno-unused-result', '-ffp-contract=fast', '--cuda-device-only', '-S']
flt = sys.argv[1] if len(sys.argv) > 1 else 'k_conv_bwd_data_v2'
srcs = ['vae_conv_v2.hip'] + (['vae_conv_tiled.hip'] if 'igemm' in flt else [])


def blocks(lines):
    cur, name = [], 'entry'
    for ln in lines:
        if re.match(r'^\.LBB\d+_\d+:', ln):
            yield name, cur
            cur, name = [], ln.split(':')[0]
        else:
            cur.append(ln.strip())
    yield name, cur


with tempfile.TemporaryDirectory() as td:
    for src in srcs:
        out = os.path.join(td, src + '.s')
        subprocess.run(['/opt/rocm/bin/hipcc', *FLAGS, os.path.join(CSRC, src), '-o', out], check=True, capture_output=True)
        text = open(out).read().split('\n')
        starts = [i for i, ln in enumerate(text) if re.match(r'^_Z\S+:', ln) and flt in ln]
        for i in starts:
            kname = text[i].split(':')[0]
            end = next(j for j in range(i, len(text)) if text[j].startswith('.Lfunc_end'))   # past early-exit s_endpgm's
            print(kname)
            tot = [0, 0]
            for bname, ins in blocks(text[i + 1:end]):
                ops = [x.split()[0] for x in ins if x and not x.startswith(';') and not x.startswith('.')]
                mf = sum(o.startswith('v_mfma') for o in ops)
                if mf < 16:
                    continue
                va = sum(o.startswith('v_') and not o.startswith('v_mfma') for o in ops)
                ds = sum(o.startswith('ds_read') for o in ops)
                wc = sum(o == 's_waitcnt' for o in ops)
                # the k-loop proper: from the first LDS operand read to the last MFMA (the block's head computes the tile's base addresses)
                a = next(k for k, o in enumerate(ops) if o.startswith('ds_read') or o.startswith('v_mfma'))
                b = max(k for k, o in enumerate(ops) if o.startswith('v_mfma'))
                vk = sum(o.startswith('v_') and not o.startswith('v_mfma') for o in ops[a:b + 1])
                tot[0] += mf
                tot[1] += va
                print('  %-10s mfma %4d  other valu %4d (k-loop %d)  ds_read %4d  s_waitcnt %4d   valu/mfma %.3f (k-loop %.3f)  waitcnt/mfma %.3f' %
                      (bname, mf, va, vk, ds, wc, va / mf, vk / mf, wc / mf))
            if tot[0]:
                print('  MFMA blocks together: valu/mfma %.3f' % (tot[1] / tot[0]))
