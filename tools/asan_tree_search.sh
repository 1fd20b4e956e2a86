#!/bin/bash
# AddressSanitizer + UBSan run of the pure decisions of the NNI tree search (iq-tree_amd/host/search_host.h) as a stand-alone
# program on the CPU: no device, nothing loaded into Python.
set -e
cd "$(dirname "$0")/.."
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -o "$D/asan_tree_search" tools/asan_tree_search.cpp
"$D/asan_tree_search"
