// Stand-in for the logging header the reference's assembly file includes: the five macros it uses.  A failed check throws.
#pragma once
#include <stdexcept>
#define FI_REF_FAIL(what) throw std::runtime_error(what)
#define CHECK_F(cond, ...) do { if (!(cond)) { FI_REF_FAIL("CHECK_F failed: " #cond); } } while (0)
#define CHECK_NOTNULL_F(ptr, ...) do { if ((ptr) == nullptr) { FI_REF_FAIL("CHECK_NOTNULL_F failed: " #ptr); } } while (0)
#define CHECK_EQ_F(a, b, ...) do { if (!((a) == (b))) { FI_REF_FAIL("CHECK_EQ_F failed: " #a " == " #b); } } while (0)
#define ABORT_F(...) FI_REF_FAIL("ABORT_F")
#define LOG_SCOPE_F(verbosity, ...) do { } while (0)
