#!/bin/bash
# timing-only variant of the library: tools/build_alt.sh <name> <hipcc flags for kernels_mfma.hip / kernels_valu4.hip / kernels_valu4w.hip ...>
# -> iq-tree_amd/lib_alt_<name>/ (git-ignored), selected at run time with IQHIP_LIB_DIR.  Results of such a build may be wrong.
# Every other object is copied from iq-tree_amd/lib (run `make` first); the libraries are linked by the Makefile's own rules.
set -e
name=$1; shift
cd "$(dirname "$0")/.."
d=iq-tree_amd/lib_alt_$name
mkdir -p $d
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -Wno-unused-value -Wno-unused-result -Iinclude"
for f in kernels_mfma kernels_valu4 kernels_valu4w; do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c iq-tree_amd/csrc/$f.hip -o $d/$f.o &
done
for o in iq-tree_amd/lib/*.o; do
  case $(basename $o .o) in
    kernels_mfma|kernels_valu4|kernels_valu4w) ;;
    *) cp -p $o $d/ ;;
  esac
done
wait
touch $d/*.o   # (newer than the sources: make links what is here and compiles nothing)
make LIBDIR=$d $d/libiqhip.so $d/libiqhost.so
echo built $d
