#!/bin/bash
# Measurement build of the library with in-kernel wall-clock stamps in the split attention kernel and in the row mat-vec
# kernel (-DL2Z_TIMELINE): llama2.zig_amd/libllama2_hip_tl.so, loaded by scripts/attn_timeline.py and
# scripts/packed_kinds_ab.py through L2Z_LIB.  Never the product library.
set -e
cd "$(dirname "$0")/../llama2.zig_amd/csrc"
make -s all
TMP=$(mktemp -d)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -DL2Z_TIMELINE"
/opt/rocm/bin/hipcc $FLAGS -c attention.hip -o "$TMP/attention_tl.o"
/opt/rocm/bin/hipcc $FLAGS -c matvec.hip -o "$TMP/matvec_tl.o"
OBJS=$(sed -n 's/^OBJS := //p' Makefile | sed 's/\battention\.o\b//;s/\bmatvec\.o\b//')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o ../libllama2_hip_tl.so "$TMP/attention_tl.o" "$TMP/matvec_tl.o" $OBJS -ldl -Wl,-rpath,/opt/rocm/lib
rm -rf "$TMP"
ls -la ../libllama2_hip_tl.so
