// The handles of the constrained-decoding C ABI (kjarni_hip.h), shared by ffi_constraint.cpp and ffi_llm.cpp.
#pragma once
#include <memory>

#include "constraint_kernels.h"

struct KjarniHipRegex {
    kjarni::ConstraintDfa dfa;
};

struct KjarniHipConstraint {
    std::unique_ptr<kjarni::DeviceConstraint> inner;
};
