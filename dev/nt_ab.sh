# Non-temporal vs plain loads in the weight gradient (profiles/r02/nt_ab.txt).
# The variants it times (nt / nont, b1nt / b1nont) were libraries built by
# dev/h3var.sh with -DNR_W3_NT / -DNR_W3_DMA_NT.  wgrad.hip no longer has those
# defines (the measured choices are fixed in wgrad3.h ld_seg and wgrad_b1.h
# kDmaAux); commit d1ec9da is the last from which the variants build.  Kept as
# the record of how the numbers were made.
set -e
mkdir -p gpurun_out
timeout -k 10 200 python dev/time_h3var.py nt,nont,nt,nont,nt,nont 20 > gpurun_out/nt_ab_h3.txt 2>&1
NR_VAR_MATH=bf16 timeout -k 10 200 python dev/time_h3var.py b1nt,b1nont,b1nt,b1nont,b1nt,b1nont 20 > gpurun_out/nt_ab_b1.txt 2>&1
