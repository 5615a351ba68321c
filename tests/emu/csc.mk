# TEST-ONLY: the CSC transpose's tile bodies (csc_core.h) on the CPU (csc_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/csc_check: csc_check.cpp $(SRC)/csc_core.h $(SRC)/common.h $(SRC)/hd.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ csc_check.cpp -lpthread
