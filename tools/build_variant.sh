#!/bin/bash
# Builds a VARIANT of libdad3d_hip.so next to (never instead of) the product library, for A/B timing on the GPU box:
#   tools/build_variant.sh <name> "<extra hipcc flags for flame_decode>" [decode source]
#   HEAD_SRC=<file> HEAD_FLAGS="-DDAD3D_HEAD_RIDE=0 ..." tools/build_variant.sh <name> ""   # a variant of the 48 + 16 kernel (flame_decode_head.hip)
# -> tools/_variants/lib_<name>.so ; use through DAD3D_LIB_PATH (dad_3dheads_amd/_lib.py). tools/_variants/ is git-ignored
# but travels with the gpurun snapshot.
set -e
root="$(cd "$(dirname "$0")/.." && pwd)"; S="$root/dad-3dheads_amd/csrc"
name="$1"; flags="$2"; src="${3:-$S/flame_decode.hip}"
H=/opt/rocm/bin/hipcc; C="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -I$S -I$root/include"
mkdir -p "$root/tools/_variants"; tmp="$(mktemp -d)"; trap 'rm -rf "$tmp"' EXIT
(cd "$S" && make -s)
$H $C $flags -x hip -c "$src" -o "$tmp/fd.o"
$H $C $flags -x hip -c "${PIPE_SRC:-$S/flame_decode_pipe.hip}" -o "$tmp/fdp.o"  # PIPE_SRC: another revision of the pipelined kernel (e.g. `git show HEAD:...` into a file)
$H $C $flags -fno-slp-vectorize -x hip -c "${SPLIT_SRC:-$S/flame_decode_split.hip}" -o "$tmp/fds.o"  # SPLIT_SRC: another revision of the bf16x3 split kernel
# HEAD_SRC / HEAD_FLAGS: another revision of the 48 + 16 kernel and / or its knobs (DAD3D_HEAD_RIDE, _RIDE_G0, _Q_AT, _DEPTH), built as the Makefile builds the unit
$H $C $flags -mllvm -amdgpu-kernarg-preload-count=14 $HEAD_FLAGS -x hip -c "${HEAD_SRC:-$S/flame_decode_head.hip}" -o "$tmp/fdh.o"
$H $C $flags -DDAD3D_DIAG_SPIN_ENV -x hip -c "$S/capi.cpp" -o "$tmp/capi.o"
# every other object of the product library as the Makefile built it (its OBJS list, minus the five compiled above)
others="$(cd "$S" && make -s -pn 2>/dev/null | sed -n 's/^OBJS *:= *//p' | head -1 | tr ' ' '\n' | grep -v -x -e flame_decode.o -e flame_decode_pipe.o -e flame_decode_head.o -e flame_decode_split.o -e capi.o | sed "s|^|$S/|")"
$H --offload-arch=gfx950 -shared -fPIC -o "$root/tools/_variants/lib_$name.so" "$tmp/fd.o" "$tmp/fdp.o" "$tmp/fdh.o" "$tmp/fds.o" "$tmp/capi.o" $others
echo "built tools/_variants/lib_$name.so"
