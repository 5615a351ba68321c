# TEST-ONLY: the quantile cuts' tile bodies (cuts_core.h) on the CPU (cuts_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/cuts_check: cuts_check.cpp $(SRC)/cuts_core.h $(SRC)/common.h $(SRC)/hd.h
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ cuts_check.cpp -lpthread
