// CommandScreen.h — `fpmash screen` (CommandScreen.h:16-60, doc/man/mash-screen.1): how much of
// each sketch of a database is in a pool of sequences, [identity, shared-hashes,
// median-multiplicity, p-value, query-ID, query-comment] per reference.
#pragma once

#include "Command.h"

namespace fpmhost {

class CommandScreen : public Command {
public:
    CommandScreen();
    int run() const override;
};

}  // namespace fpmhost
