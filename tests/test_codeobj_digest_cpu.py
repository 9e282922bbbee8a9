"""tools/codeobj_digest.py as a gate: its digests are a function of the device code alone.  The same kernel compiled in two
directories (clang's per-compile ``__hip_cuid_<hash>`` symbol differs, and with it the name tables) has one digest; one
changed constant has another."""
import importlib.util
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = '''#include <hip/hip_runtime.h>
__global__ void scale_kernel(float *y, const float *x, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = x[i] * %s;
}
'''


@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('codeobj_digest', os.path.join(ROOT, 'tools', 'codeobj_digest.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def libs(tmp_path_factory):
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = {}
    for tag, const in (('a', '3.0f'), ('b', '3.0f'), ('c', '5.0f')):
        d = tmp_path_factory.mktemp('digest_' + tag)
        src, lib = str(d / 'scale.hip'), str(d / 'libscale.so')
        with open(src, 'w') as f:
            f.write(KERNEL % const)
        subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-fPIC', '-shared', src, '-o', lib], check=True, cwd=str(d))
        out[tag] = lib
    return out


def _cuid(tool, lib):
    from workoutdetector_amd.codeobj import _gfx950_elfs
    elf, = _gfx950_elfs(lib)
    strtab = dict(tool.sections(elf))['.strtab']
    return [s for s in strtab.split(b'\0') if s.startswith(b'__hip_cuid_')]


def test_same_code_from_two_directories_has_one_digest(tool, libs):
    assert _cuid(tool, libs['a']) and _cuid(tool, libs['a']) != _cuid(tool, libs['b'])     # the builds do differ in the cuid
    da, db = tool.digests(libs['a']), tool.digests(libs['b'])
    assert len(da) == 1 and da == db
    assert tool.kernels(libs['a']) == tool.kernels(libs['b'])
    assert list(tool.kernels(libs['a'])) == ['scale_kernel']


def test_one_changed_constant_changes_the_digest(tool, libs):
    assert tool.digests(libs['a']) != tool.digests(libs['c'])
    assert tool.kernels(libs['a']) != tool.kernels(libs['c'])


def test_two_libraries_mode_exit_status(libs):
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'codeobj_digest.py')]
    same = subprocess.run(cmd + [libs['a'], libs['b']], capture_output=True, text=True)
    assert same.returncode == 0 and 'scale_kernel' not in same.stdout, same.stdout + same.stderr
    diff = subprocess.run(cmd + [libs['a'], libs['c']], capture_output=True, text=True)
    assert diff.returncode == 1 and 'scale_kernel' in diff.stdout, diff.stdout + diff.stderr
