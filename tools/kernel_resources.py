"""Per-kernel resource report for csrc/*.hip files (gfx950, device side).

    python tools/kernel_resources.py coinstac_dinunet_amd/ops/csrc/conv3d.hip \
        [more.hip ...] [--filter wgrad] [-I extra/include]

Compiles each file with the flags of ops/build.py plus
`--cuda-device-only -Rpass-analysis=kernel-resource-usage` and prints one
line per kernel: VGPRs, AGPRs, LDS bytes per block, private-segment
(scratch) bytes per lane, occupancy in waves per SIMD. Only the compiler's
resource remarks are read, never the instruction stream.

A non-zero private segment on a hot kernel means a register array went to
memory (a runtime index into it is the usual cause) or the kernel spills.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

_FIELDS = {
    'VGPRs': 'vgprs',
    'AGPRs': 'agprs',
    'ScratchSize [bytes/lane]': 'private',
    'Occupancy [waves/SIMD]': 'occupancy',
    'LDS Size [bytes/block]': 'lds',
}
_REMARK = re.compile(r'remark:\s+(.+?): (\S+)\s*'
                     r'\[-Rpass-analysis=kernel-resource-usage\]')


def parse_remarks(text):
    """[{name, vgprs, agprs, lds, private, occupancy}] from hipcc stderr."""
    kernels, cur = [], None
    for line in text.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == 'Function Name':
            cur = {'name': val}
            kernels.append(cur)
        elif cur is not None and key in _FIELDS:
            cur[_FIELDS[key]] = int(val)
    return kernels


def _demangle(names):
    filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if filt is None:
        for d in ('/opt/rocm/llvm/bin', '/opt/rocm/lib/llvm/bin'):
            if os.path.exists(os.path.join(d, 'llvm-cxxfilt')):
                filt = os.path.join(d, 'llvm-cxxfilt')
                break
    if filt is None or not names:
        return list(names)
    out = subprocess.run([filt], input='\n'.join(names), text=True,
                         capture_output=True, check=True).stdout.splitlines()
    # "void kern<32, 1>(args...)" -> "kern<32, 1>"
    short = []
    for s in out:
        s = re.sub(r'^void ', '', s)
        m = re.match(r'_Z(\d+)', s)   # a type the demangler does not know
        if m:
            s = s[m.end():m.end() + int(m.group(1))]
        depth = 0
        for i, c in enumerate(s):
            depth += c == '<'
            depth -= c == '>'
            if c == '(' and depth == 0:
                s = s[:i]
                break
        short.append(s)
    return short


def kernel_resources(src, extra_includes=()):
    """Compile one .hip file device-only; return its kernels' resources."""
    from coinstac_dinunet_amd.ops.build import compile_flags
    with tempfile.TemporaryDirectory() as tmp:
        cmd = (['hipcc', '-c', src, '-o', os.path.join(tmp, 'dev.o'),
                '--cuda-device-only',
                '-Rpass-analysis=kernel-resource-usage']
               + compile_flags() + [f'-I{d}' for d in extra_includes])
        p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f'hipcc failed on {src}:\n{p.stderr[-4000:]}')
    kernels = parse_remarks(p.stderr)
    for k, name in zip(kernels, _demangle([k['name'] for k in kernels])):
        k['mangled'], k['name'] = k['name'], name
        k['file'] = os.path.basename(src)
    return kernels


def report(sources, extra_includes=(), name_filter=None):
    with ThreadPoolExecutor(max_workers=min(4, len(sources))) as ex:
        per_file = list(ex.map(
            lambda s: kernel_resources(s, extra_includes), sources))
    rows = [k for ks in per_file for k in ks]
    if name_filter:
        rows = [k for k in rows if name_filter in k['name']
                or name_filter in k['mangled']]
    return rows


def format_row(k):
    return (f"{k['file']:<20} vgpr={k.get('vgprs', -1):<4} "
            f"agpr={k.get('agprs', -1):<4} lds={k.get('lds', -1):<6} "
            f"private={k.get('private', -1):<5} "
            f"occ={k.get('occupancy', -1):<2} {k['name']}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('sources', nargs='+', help='csrc/*.hip files')
    ap.add_argument('-I', dest='includes', action='append', default=[],
                    help='extra include directory')
    ap.add_argument('--filter', default=None,
                    help='only kernels whose name contains this')
    args = ap.parse_args()
    for k in report(args.sources, args.includes, args.filter):
        print(format_row(k))


if __name__ == '__main__':
    main()
