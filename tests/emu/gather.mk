# TEST-ONLY: the row-gather tile bodies (gather_core.h) on the CPU (gather_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/gather_check: gather_check.cpp $(SRC)/gather_core.h $(SRC)/common.h $(SRC)/hd.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ gather_check.cpp -lpthread
