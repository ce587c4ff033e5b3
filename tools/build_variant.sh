#!/bin/bash
# build a kernel-library variant into build_var/<name>.so with extra -D flags:  tools/build_variant.sh name -DFOO=1 ...
# (build_var/ is git-ignored; select a variant with CSTP_LIB_PATH=build_var/<name>.so)
# The sources are the build entry point's own list, so the variant exports every symbol _lib.load() checks for.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build_var
sources=$(python3 -c 'import __graft_entry__ as e; print(" ".join("cstp_amd/csrc/" + s for s in e.SOURCES))')
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -shared -Iinclude -Icstp_amd/csrc "$@" -o build_var/$name.so $sources
echo built build_var/$name.so
