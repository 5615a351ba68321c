# TEST-ONLY: the tile prologue's chunk list and decoder tables on the CPU (chunk_guess_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/chunk_guess_check: chunk_guess_check.cpp $(wildcard $(SRC)/*.h)
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -g -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
	  -I$(SRC) -I../../include -o $@ chunk_guess_check.cpp -lpthread
