# TEST-ONLY CPU emulator of the whitespace-delimiter / integer-label CSV tile
# bodies (see emu_csv_ws.cpp): make -C tests/emu -f csv_ws.mk
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
all: _build/emu_csv_ws_asan
_build/emu_csv_ws_asan: emu_csv_ws.cpp emu.cpp $(wildcard $(SRC)/*.h) ../../include/dmlc_amd.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ emu_csv_ws.cpp -lpthread
.PHONY: all
