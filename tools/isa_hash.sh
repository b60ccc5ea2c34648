#!/bin/bash
# sha256 of the gfx950 disassembly of every kernel in a shape object (symbol by symbol): "did this source change alter any code?"
#   tools/isa_hash.sh <object.o> > hashes.txt
B=/opt/rocm/lib/llvm/bin; tmp=$(mktemp -d)
$B/llvm-objcopy --dump-section .hip_fatbin=$tmp/fat.bin $1 && $B/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/fat.bin --output=$tmp/k.co --unbundle
$B/llvm-objdump -d $tmp/k.co | python3 -c "
import sys, re, hashlib
cur=None; t={}
for line in sys.stdin:
    m=re.match(r'^[0-9a-f]+ <(\S+)>:', line)
    if m: cur=m.group(1); t[cur]=[]; continue
    # ('...' is the zero padding up to the next symbol's alignment: it follows what comes after the kernel, not the kernel)
    if cur and re.match(r'\s+\S', line) and line.strip() != '...':
        # drop addresses / encodings / resolved branch targets: the instruction text only
        t[cur].append(re.sub(r'\s*//.*', '', line).strip())
for k in sorted(t):
    # (and the displacement of a call target, s_getpc_b64 / s_add_u32 <rel32 lo> / s_addc_u32 <rel32 hi>: where the callee was laid out)
    for i, l in enumerate(t[k]):
        if l.startswith('s_getpc_b64'):
            for j in (i + 1, i + 2):
                if j < len(t[k]) and re.match(r's_add(c)?_u32 ', t[k][j]): t[k][j] = re.sub(r', (0x[0-9a-f]+|-?\d+)$', ', <rel32>', t[k][j])
    # (so is the run of s_nop 0 behind a symbol's last instruction: as many as the next symbol's alignment asks for)
    while t[k] and t[k][-1] == 's_nop 0': t[k].pop()
    print(hashlib.sha256(''.join(l + '\n' for l in t[k]).encode()).hexdigest()[:16], k)
"
rm -rf $tmp
