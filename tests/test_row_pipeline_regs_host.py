"""What the row look-ahead of param_grad_df_split_kernel (csrc/gp_backward.hip, chunk_rows_ahead) is for, read off the built library
without a GPU: no private segment, no spilled vector register, and at most 256 vector registers -- two workgroups per CU.  The loop
leans on a handful of compiler-steering devices; a toolchain that stops honouring them shows here first."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_parameter_sums_keep_no_scratch_and_two_workgroups_per_cu():
    lib = os.path.join(ROOT, 'vae-gp-ode_amd', 'libgpode_hip.so')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_regs.py'), lib, 'param_grad_df_split_kernel'],
                         capture_output=True, text=True, check=True).stdout
    rows = [l for l in out.split('\n') if 'param_grad_df_split_kernel<6>' in l]
    print(out)
    assert len(rows) == 1, out
    m = re.match(r'vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+\d+ lds\s+\d+ scratch\s+(\d+) spill_v\s+(\d+)', rows[0])
    vgpr, agpr, scratch, spill_v = map(int, m.groups())
    assert scratch == 0 and spill_v == 0, rows[0]
    assert vgpr + agpr <= 256, rows[0]
