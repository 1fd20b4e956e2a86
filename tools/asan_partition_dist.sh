#!/bin/bash
# AddressSanitizer + UBSan run of the plain C++ side of the starting tree of a partitioned alignment (the chunk and cell-list
# layout of iq-tree_amd/csrc/partpair_layout.h, the weighted mean of iq-tree_amd/host/supertree_brlen.h) as a stand-alone
# program on the CPU: no device, nothing loaded into Python.
set -e
cd "$(dirname "$0")/.."
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -o "$D/asan_partition_dist" tools/asan_partition_dist.cpp
"$D/asan_partition_dist"
