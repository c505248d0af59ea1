// The handles of the grammar C ABI (kjarni_hip.h), shared by ffi_grammar.cpp, ffi_llm.cpp and ffi_chat.cpp.
#pragma once
#include <memory>

#include "grammar_kernels.h"

struct KjarniHipGrammar {
    kjarni::Grammar grammar;
};

struct KjarniHipGrammarConstraint {
    std::unique_ptr<kjarni::DeviceGrammar> inner;
};
