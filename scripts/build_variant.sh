#!/bin/bash
# A/B builds: scripts/build_variant.sh <name> <sed-expr> <file.hip> [<sed-expr> <file.hip> ...]
# compiles patched copies of the named sources (everything else reuses uformer_amd/lib/*.o) into ab/<name>/libuformer_hip.so;
# select it at run time with UFORMER_HIP_LIB=ab/<name>/libuformer_hip.so.  The source list and the per-file flags are build()'s
# (__graft_entry__.SOURCES / EXTRA_FLAGS), so a variant differs from the shipped library in the patch alone.
#
# Diagnostic build: scripts/build_variant.sh --stamps [<name>]   (default name: stamps)
# compiles the sources that carry in-kernel instrumentation (uf_stamps.h: Census, stamp(), role and phase timers) with -DUF_STAMPS=1 into
# ab/<name>/libuformer_hip.so, beside the shipped library, which has none and whose uf_debug_set_tbuf refuses a buffer.  The stamp and census
# commands of scripts/ubench.py need it: UFORMER_HIP_LIB=ab/stamps/libuformer_hip.so python scripts/ubench.py stamps ...
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
STAMPED="uf_core.hip uf_lngemm.hip uf_leff2.hip uf_attnblk.hip"      # every source that reads UF_STAMPS
defs=""
if [ "$1" = "--stamps" ]; then
    shift; defs="-DUF_STAMPS=1"
    [ $# -le 1 ] || { echo "build_variant.sh --stamps [<name>]: takes no patch pairs (got: ${*:2})" >&2; exit 2; }
    set -- "${1:-stamps}"
fi
name=$1; shift
out=$R/ab/$name; mkdir -p $out; objs=""
declare -A patched
if [ -n "$defs" ]; then
    for f in $STAMPED; do cp $R/uformer_amd/csrc/$f $out/$f; patched[$f]=1; done
fi
while [ $# -ge 2 ]; do
    expr=$1; f=$2; shift 2
    src=$out/$f; [ -f $src ] || cp $R/uformer_amd/csrc/$f $src
    sed -i "$expr" $src; patched[$f]=1
done
for f in $(cd $R && python -c "import __graft_entry__ as g; print(' '.join(g.SOURCES))"); do
    if [ -n "${patched[$f]}" ]; then
        extra=$(cd $R && python -c "import sys, __graft_entry__ as g; print(' '.join(g.EXTRA_FLAGS.get(sys.argv[1], [])))" $f)
        /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $extra $defs -I$R/uformer_amd/csrc -c $out/$f -o $out/${f%.hip}.o    # -I: the copy's "uf_*.h" includes
        objs="$objs $out/${f%.hip}.o"
    else
        objs="$objs $R/uformer_amd/lib/${f%.hip}.o"
    fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libuformer_hip.so $objs
echo "built $out/libuformer_hip.so"
