#!/bin/bash
# Usage: tools/loop_spill_check.sh [csrc directory] [extra hipcc flags]      (default: this tree's csrc)
# Compiles that directory's rrtx_api.hip for gfx950 (CPU only, ~1 min) and reports, for the three rrt_star_kernel_v2
# instantiations, the resource-usage remarks, and for every streaming loop of rppk2t::rrt_star_kernel_v2 the lines per slot,
# the scratch instructions and the full s_waitcnt vmcnt(0) drains inside it: a register-allocation regression of the hot
# loop shows here before any GPU time is spent.  Run it on two directories (a checkout of the parent commit
# and this tree) to compare them; KEEP_ASM=<file> keeps the device assembly.
REPO=$(cd "$(dirname "$0")/.." && pwd)
SRC=$REPO/robotics-path-planning_amd/csrc
if [ -n "$1" ] && [ "${1#-}" = "$1" ]; then   # a first argument that is no flag names the directory
  [ -f "$1/rrtx_api.hip" ] || { echo "usage: $0 [csrc directory] [extra hipcc flags]   ($1 holds no rrtx_api.hip)" >&2; exit 2; }
  SRC=$(cd "$1" && pwd); shift
fi
D=$(mktemp -d); trap 'rm -rf "$D"' EXIT; cp $SRC/* $D/
cd $D && sed -i "s#\"../../include/rrtx.h\"#\"$REPO/include/rrtx.h\"#" rrtx_api.hip $(ls rrtx_host.h 2>/dev/null)
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wno-parentheses-equality -Wno-unused-value "$@" --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o $D/o.s rrtx_api.hip 2> $D/err.txt
grep -E "error" $D/err.txt | head -3
for ns in 5rppk2 6rppk2s 6rppk2t; do
  echo -n "${ns:1}: "
  grep -A12 "Function Name: _ZN${ns}18rrt_star_kernel_v2EN4rppk3CtxEi " $D/err.txt | grep -E "VGPRs Spill|ScratchSize|SGPRs Spill|Occupancy|LDS Size" | sed -e 's/.*remark: *//' -e 's/ *\[-Rpass.*//' | tr '\n' ';'; echo
done
[ -n "$KEEP_ASM" ] && cp $D/o.s "$KEEP_ASM"
L=$(grep -n "^_ZN6rppk2t18rrt_star_kernel_v2EN4rppk3CtxEi:" $D/o.s | cut -d: -f1)
awk -v l=$L 'NR>=l' $D/o.s | awk '/s_endpgm/{print; exit} {print}' > $D/k.s
python3 - $D/k.s <<'PY'
import sys,re
L=open(sys.argv[1]).read().split('\n')
loads=[i for i,l in enumerate(L) if 'global_load_dwordx4' in l and ' nt' in l]
# group loads: consecutive loads closer than 60 lines = prologue group; loop loads follow
groups=[]; cur=[loads[0]]
for a,b in zip(loads,loads[1:]):
    if b-a<60: cur.append(b)
    else: groups.append(cur); cur=[b]
groups.append(cur)
# a streaming loop = prologue group (>=4 loads) followed by singles
i=0
while i<len(groups):
    g=groups[i]
    if len(g)>=2:
        j=i+1; last=g[-1]
        while j<len(groups) and len(groups[j])==1: last=groups[j][0]; j+=1
        if j>i+1:
            rng=L[g[-1]:last+1]
            sc=[l for l in rng if 'scratch_' in l]
            v0=[l for l in rng if 's_waitcnt vmcnt(0)' in l]
            print("loop lines %d-%d: %d lines/slot, scratch ops %d, vmcnt(0) %d"%(g[-1],last,(last-g[-1])//max(1,(j-i-1)),len(sc),len(v0)))
        i=j
    else: i+=1
PY
