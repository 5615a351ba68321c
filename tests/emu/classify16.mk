# TEST-ONLY: the front half's piece classifier and quad exchange on the CPU (classify16_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/classify16_check: classify16_check.cpp $(wildcard $(SRC)/*.h)
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ classify16_check.cpp
