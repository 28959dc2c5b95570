// em_device.hpp -- device-resident EM refinement of vanishing points, one workgroup per image.
//
// MI355X-first design: the whole EM of one image (setup, E-step, N x N smoothing, M-step,
// split / merge / finalisation control flow) runs inside ONE persistent workgroup, so an
// iteration costs barriers instead of kernel launches and the only HBM stream that matters is
// the fp64 N x N line-similarity matrix read once per E-step (B_EM).  Hundreds
// of images run concurrently (one per workgroup), which is where the throughput comes from.
//
// All arithmetic is fp64 (fp32 only where the reference is fp32: the prior weights).  The
// translation unit is compiled with -ffp-contract=off so that products and sums round like the
// reference's separate NumPy ufunc calls; the two bandwidth-bound accumulation loops use an
// explicit fma().
//
// Conventions: every VPK_DEVFN below is called by ALL threads of the workgroup with uniform
// arguments, expects its inputs to be visible (a barrier has happened) and ends with a barrier.
// Citations are file:line under /root/reference.
//
// This file is the umbrella: the phases live in the em_*.hpp parts included below, in the order their definitions need.
#ifndef VPK_EM_DEVICE_HPP_
#define VPK_EM_DEVICE_HPP_

#include "em_ctx.hpp"
#include "em_linalg.hpp"
#include "em_setup.hpp"
#include "em_estep.hpp"
#include "em_smooth.hpp"
#include "em_assign.hpp"
#include "em_mstep.hpp"
#include "em_vpset.hpp"
#include "em_run.hpp"

#endif
