"""Build ``ffcv_amd/libffcv_hip.so`` for gfx950 in-tree (hipcc).

    python -m ffcv_amd._build [--force]

The .so is git-ignored but travels to the GPU box with the gpurun snapshot.

A/B and diagnostic variants (tools/build_variant.sh) are the same recipe with
another output and extra compiler flags after ``--``:

    python -m ffcv_amd._build --out build/ab/stop4.so -- -DK1_STOP=4
"""
import argparse
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OUT = os.path.join(HERE, 'libffcv_hip.so')
SOURCES = ['ffcv_common.hip', 'ffcv_rrc.hip', 'ffcv_jpeg.hip', 'ffcv_host.hip', 'ffcv_cpu_jpeg.hip',
           'ffcv_color.hip', 'ffcv_mixup.hip', 'ffcv_poison.hip', 'ffcv_gather.hip', 'ffcv_rrc_images.hip',
           'ffcv_blur.hip', 'ffcv_hue.hip', 'ffcv_affine.hip', 'ffcv_tone.hip', 'ffcv_standalone.hip',
           'ffcv_simple_aug.hip', 'ffcv_sharpness.hip', 'ffcv_policy.hip', 'ffcv_cutmix.hip',
           'ffcv_erase.hip', 'ffcv_randaugment.hip']
HEADERS = ['api_internal.h', 'device_common.h', 'diag_hooks.h', 'color_common.h', 'blur_common.h', 'hue_common.h',
           'affine_common.h', 'tone_common.h', 'poison_common.h', 'jpeg_defs.h', 'jpeg_entropy.h', 'jpeg_idct.h',
           'jpeg_color_resize.h', 'lds_stage.h', 'resize_out.h', 'sharpness_common.h', 'band_tiles.h',
           'erase_common.h']
ARCH = os.environ.get('PYTORCH_ROCM_ARCH', 'gfx950').split(';')[0]

FLAGS = ['--offload-arch=' + ARCH, '-O3', '-fPIC', '-shared', '-std=c++17',
         # bit-exact float paths (INTER_AREA taps, crop draws): no FMA contraction
         '-ffp-contract=off', '-fno-fast-math', '-Wall', '-Wno-unused-function']


def _stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS]
    deps.append(os.path.join(os.path.dirname(HERE), 'include', 'ffcv_hip.h'))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, out=None, extra_flags=()):
    """The product library, rebuilt when a source is newer; or, with `out`
    (and `extra_flags`), a variant at that path, always built."""
    if out is None:
        if not force and not _stale():
            return OUT
        out = OUT
    else:
        out = os.path.abspath(out)
        os.makedirs(os.path.dirname(out), exist_ok=True)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc] + FLAGS + list(extra_flags) + ['-o', out + '.tmp'] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    os.replace(out + '.tmp', out)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--force', action='store_true', help='rebuild the product library even when it is up to date')
    ap.add_argument('--out', help='build a variant at this path instead of the product library')
    ap.add_argument('extra_flags', nargs='*', help='extra compiler flags (after --)')
    a = ap.parse_args()
    print(build(force=a.force, verbose=True, out=a.out, extra_flags=a.extra_flags))
