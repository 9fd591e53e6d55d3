# TEST INFRASTRUCTURE build recipe of the RDS decoding chain's oracle and reference harness (run from oracle/: make -f rds_chain.mk ...).
#
#   make -f rds_chain.mk oracle   -> liboracle_rds.so       our C restatement of the chain (rds_chain.c), runs anywhere
#   make -f rds_chain.mk ref      -> _ref/fm_rds_db_dump    the reference's own src/rds_decoder/*.cpp (compiled where they lie, nothing
#                                                            copied) behind our dump harness rds_db_dump.cpp; only where $(REF) is mounted
# Flags as Makefile's: the oracle without fast-math, the reference with its `gcc` preset's.
REF      ?= /root/reference
RSRC     := $(REF)/src
REF_MARCH ?= x86-64-v3
OUT      := _ref
CXX      ?= g++
CC       ?= gcc

.PHONY: all oracle ref
all: oracle

oracle: liboracle_rds.so

liboracle_rds.so: rds_chain.c rds_chain.h
	$(CC) -O2 -std=c11 -fPIC -Wall -Wextra -shared rds_chain.c -o $@

ifneq ($(wildcard $(RSRC)/rds_decoder/rds_decoding_chain.h),)
ref: $(OUT)/fm_rds_db_dump

$(OUT)/fm_rds_db_dump: rds_db_dump.cpp $(wildcard $(RSRC)/rds_decoder/*.cpp)
	@mkdir -p $(OUT)
	$(CXX) -std=c++17 -O2 -ffast-math -march=$(REF_MARCH) -I$(RSRC) rds_db_dump.cpp $(wildcard $(RSRC)/rds_decoder/*.cpp) -o $@
else
ref:
	@echo "reference tree $(REF) not mounted: keeping prebuilt $(OUT)/fm_rds_db_dump (if any)"
endif
