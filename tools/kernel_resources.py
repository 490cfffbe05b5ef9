"""Per-kernel register / LDS / scratch usage of the built library (AMDGPU code-object metadata).
    python tools/kernel_resources.py [pattern] [lib]
    python tools/kernel_resources.py --rnn-budget
--rnn-budget lists the sequence-persistent recurrent kernels (csrc/lstm*.hip, gru*.hip), single and paired, and exits
with 1 unless every one of them is there - 28 single, 28 paired - without spills or scratch and, for the 1,024-thread
128-unit kernels, within the 128 VGPRs (AGPRs included) that DESIGN 4.4's launch bound leaves a lane."""
import re, subprocess, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
budget = '--rnn-budget' in sys.argv[1:]
argv = [a for a in sys.argv if a != '--rnn-budget']
pat = '_seq_' if budget else (argv[1] if len(argv) > 1 else '')
lib = argv[2] if len(argv) > 2 else os.path.join(ROOT, 'rl_games_amd', 'librlg_hip.so')
tmp = '/tmp/_rlg_co'
os.makedirs(tmp, exist_ok=True)
import glob
objs = sorted(glob.glob(os.path.join(ROOT, 'rl_games_amd', 'csrc', 'build', '*.o'))) if len(argv) <= 2 else [lib]
out = ''
for o in objs:
    fat, co = f'{tmp}/fat.bin', f'{tmp}/dev.co'
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    if subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-objcopy', '--dump-section', f'.hip_fatbin={fat}', o],
                      capture_output=True).returncode != 0:
        continue                       # (an object without device code)
    subprocess.run(['/opt/rocm/lib/llvm/bin/clang-offload-bundler', '--unbundle', '--type=o', f'--input={fat}',
                    '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--output={co}'], check=True)
    out += subprocess.run(['/opt/rocm/lib/llvm/bin/llvm-readelf', '--notes', co], capture_output=True, text=True).stdout
cur = {}
rows = []
for line in out.splitlines():
    m = re.match(r'\s+\.(\w+):\s+(.*)', line) or re.match(r'\s+- \.(\w+):\s+(.*)', line)
    if not m:
        continue
    k, v = m.group(1), m.group(2).strip()
    if k == 'agpr_count' and cur.get('name'):
        pass
    if k in ('agpr_count', 'vgpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size',
             'vgpr_spill_count', 'sgpr_spill_count', 'name', 'symbol'):
        cur[k] = v
    if k == 'wavefront_size':
        rows.append(cur); cur = {}
# 28 = 2 cells x 2 directions x (6 narrow instantiations: H 16 at tile 16, H 32 at tiles 16 / 8, H 64 at tiles 16 / 8 / 4 -
# rnn_seq.hpp's launch_narrow_sb - + 1 wide kernel), once as single and once as paired kernels
over, seen = [], {'single': 0, 'paired': 0}
for r in rows:
    n = r.get('name', '?')
    d = subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()
    d = re.sub(r'\(.*', '', d)
    if pat and pat not in d:
        continue
    print(f"{d[:70]:70s} vgpr {r.get('vgpr_count','?'):>4} agpr {r.get('agpr_count','?'):>4} sgpr {r.get('sgpr_count','?'):>4} "
          f"scratch {r.get('private_segment_fixed_size','?'):>5} lds {r.get('group_segment_fixed_size','?'):>6} "
          f"vspill {r.get('vgpr_spill_count','0')} sspill {r.get('sgpr_spill_count','0')}")
    if budget:
        seen['paired' if '_pair_kernel' in d else 'single'] += 1
        regs = int(r.get('vgpr_count', 0)) + int(r.get('agpr_count', 0))
        if (int(r.get('private_segment_fixed_size', 0)) or int(r.get('vgpr_spill_count', 0))
                or int(r.get('sgpr_spill_count', 0)) or ('_wide_' in d and regs > 128)):
            over.append(d)
if budget:
    print(f"{seen['single']} single and {seen['paired']} paired kernels; outside the budget: {over or 'none'}")
    sys.exit(0 if not over and seen == {'single': 28, 'paired': 28} else 1)
