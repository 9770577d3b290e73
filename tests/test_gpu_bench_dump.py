"""A plain `bench.py` run: the result line reports the --steps it timed and carries none of the --full sections, and
--dump-outputs writes what the last timed step computed as float .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('mode', ['elbo', 'integrator'])
def test_plain_run_dumps_the_last_step(mode, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--workload', 'cfg1', '--mode', mode, '--steps', '3',
                        '--warmup', '1', '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['metric'] == 'latent_trajectories_per_sec'
    assert not {'roofline', 'cpu_baseline', 'extra'} & set(line), sorted(line)
    out = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in out.values())
    if mode == 'integrator':
        assert set(out) == {'zt'} and out['zt'].shape == (32, 16, 6)
    else:
        assert out['loss'].shape == () and 'state.vae.decoder.decnn.7.weight' in out and 'grad.vae.decoder.decnn.7.weight' in out
        assert out['grad.flow.odefunc.diffeq.Us_sqrt.optvar'].shape == (6, 5050)
