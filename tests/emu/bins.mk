# TEST-ONLY: the CSR -> bin codes tile body (bins_core.h) on the CPU (bins_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/bins_check: bins_check.cpp $(SRC)/bins_core.h $(SRC)/dense_core.h $(SRC)/common.h $(SRC)/hd.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ bins_check.cpp -lpthread
