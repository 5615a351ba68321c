# TEST-ONLY: the number catalogue through the host-compiled window decoders (numcat_check.cpp).
CXX ?= g++
SRC := ../../dmlc-core_amd/csrc
_build/numcat_check: numcat_check.cpp $(wildcard $(SRC)/*.h)
	@mkdir -p _build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -I$(SRC) -I../../include -o $@ numcat_check.cpp
