#!/usr/bin/env bash
# isa_digest.sh <file.hip> [more.hip ...]: print "sha256  lines  file" of each file's gfx950 assembly, compiled with the
# flags build() uses for a file of that name.  Two sources with equal digests produce identical device code (needs no GPU).
# The __hip_cuid_<hash> symbol hashes the source text, so it is replaced by a fixed token first.
set -euo pipefail
REPO="$(cd "$(dirname "$0")/.." && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
for f in "$@"; do
    extra=$(cd "$REPO" && python -c "import sys, __graft_entry__ as g; print(' '.join(g.EXTRA_FLAGS.get(sys.argv[1], [])))" "$(basename "$f")")
    # shellcheck disable=SC2086
    asm=$("$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC $extra --cuda-device-only -S "$f" -o - | sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g')
    printf '%s  %s  %s\n' "$(printf '%s\n' "$asm" | sha256sum | cut -d' ' -f1)" "$(printf '%s\n' "$asm" | wc -l)" "$f"
done
