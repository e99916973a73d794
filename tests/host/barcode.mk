# The barcode demultiplexer's HIP-free host code under the sanitizers (CPU only): make -C tests/host -f barcode.mk asan
CXX ?= g++
GOLDEN ?= ../golden/barcode
asan: bin/barcode_host_asan
	ASAN_OPTIONS=abort_on_error=1:detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 ./bin/barcode_host_asan $(GOLDEN)
bin/barcode_host_asan: barcode_host_test.cpp ../../pangea-plus_amd/csrc/barcode_host.hpp
	mkdir -p bin && $(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all barcode_host_test.cpp -o $@
