#!/bin/bash
# gecm_layout_make and gecm_layout_free of libgecm (host/gecm_mod.c) under AddressSanitizer + UBSan (CPU only; a program
# of its own).
set -e
cd "$(dirname "$0")/.."
H=avx-ecm_amd/host
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
gcc -O1 -g -std=gnu11 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -Wall -Wextra tools/layout_sanitize.c $H/gecm_mod.c $H/mpl.c -lpthread -lm -o "$tmp/gecm_layout_sanitize"
ASAN_OPTIONS=detect_leaks=1 "$tmp/gecm_layout_sanitize"
