/* Stands in for the reference's utility.h: its debug assert, always on here. */
#ifndef REF_QDISC_SHIM_UTILITY_H
#define REF_QDISC_SHIM_UTILITY_H

#include <assert.h>

#define utility_debugAssert(expr) assert(expr)

#endif
