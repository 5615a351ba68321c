# TEST-ONLY: the CSR -> dense tile body (dense_core.h) on the CPU (dense_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/dense_check: dense_check.cpp $(SRC)/dense_core.h $(SRC)/common.h $(SRC)/hd.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ dense_check.cpp -lpthread
