#!/bin/bash
# AddressSanitizer + UBSan run of the plain C++ side of the parsimony forest (the addition orders and the duplicate filter of
# iq-tree_amd/host/search_host.h; slot bases, chunk sizes and merged segment lists of iq-tree_amd/host/pars_forest_plan.h) as
# a stand-alone program on the CPU: no device, nothing loaded into Python.
set -e
cd "$(dirname "$0")/.."
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -o "$D/asan_pars_forest" tools/asan_pars_forest.cpp
"$D/asan_pars_forest"
