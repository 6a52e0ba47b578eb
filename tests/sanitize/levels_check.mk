# ASan + UBSan build of levels_check: tpt_wide_tree_levels (a refit's level ranges) over the
# wide-tree builder's own trees and over corrupted links.  CPU only: never built for or run on
# the GPU box.
#   make -f levels_check.mk && ./levels_check
CXX      ?= g++
HOST     := ../../tinypathtracer_amd/csrc/host
SAN      := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
CXXFLAGS := -O1 -g -std=c++17 -Wall $(SAN) -I../../include -I$(HOST)

levels_check: levels_check.cpp $(HOST)/wide_bvh.cpp $(HOST)/tpt_internal.hpp
	$(CXX) $(CXXFLAGS) -o $@ levels_check.cpp $(HOST)/wide_bvh.cpp -lpthread

clean:
	rm -f levels_check
.PHONY: clean
