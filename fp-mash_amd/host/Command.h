// Command.h — the reference's plugin surface (Command.h:26-136, CommandList.cpp:88-109):
// a Command owns an option registry, parses argv, and runs.  Commands register
// in main.cpp exactly as mash.cpp:23-37 does for the hot-path verbs.
#pragma once

#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace fpmhost {

class Command {
public:
    struct Option {
        enum Type { Boolean, Number, Integer, Size, File, String };
        Type type = Boolean;
        std::string identifier, category, description, argument, argumentDefault;
        double argumentMin = 0, argumentMax = 0;
        bool active = false;
        bool changed = false;
        Option() = default;
        Option(Type t, const std::string &id, const std::string &cat, const std::string &desc,
               const std::string &def = "", double mn = 0, double mx = 0);
        void setArgument(const std::string &a);
        double getArgumentAsNumber() const;
    };

    Command();
    virtual ~Command() = default;
    int run(int argc, const char **argv);
    virtual int run() const = 0;
    void print() const;
    const Option &getOption(const std::string &name) const { return options.at(name); }
    bool hasOption(const std::string &name) const { return options.count(name) > 0; }

    std::string name, summary, description, argumentString;

protected:
    void addOption(const std::string &name, const Option &o);
    void useOption(const std::string &name);
    void useSketchOptions();

    std::map<std::string, Option> options;
    std::map<std::string, Option> optionsAvailable;
    std::map<std::string, std::string> optionNamesByIdentifier;
    std::map<std::string, std::vector<std::string>> optionNamesByCategory;
    std::vector<std::string> categories;
    std::map<std::string, std::string> categoryDisplayNames;
    std::vector<std::string> arguments;

private:
    void addAvailableOption(const std::string &name, const Option &o);
    void addCategory(const std::string &name, const std::string &display);
};

class CommandList {
public:
    explicit CommandList(const std::string &name) : name(name) {}
    ~CommandList();
    void addCommand(Command *c) { commands[c->name] = c; }
    int run(int argc, const char **argv);

private:
    void print() const;
    std::string name;
    std::map<std::string, Command *> commands;
};

class CommandSketch : public Command {
public:
    CommandSketch();
    int run() const override;
};

class CommandDistance : public Command {
public:
    CommandDistance();
    int run() const override;
};

class CommandInfo : public Command {
public:
    CommandInfo();
    int run() const override;
};

class CommandPaste : public Command {
public:
    CommandPaste();
    int run() const override;
};

class CommandTriangle : public Command {
public:
    CommandTriangle();
    int run() const override;
};

// sketchParameterSetup (sketchParameterSetup.cpp:9-126)
struct Parameters;
int sketchParameterSetup(Parameters &p, const Command &c);

// What the verbs' run() functions share.
class Sketch;
// containsMSH / containsTXT (CommandDistance.cpp:454-476): substring test on the last file
bool containsSub(const std::vector<std::string> &v, const char *s);
// args[first..) as input files; with `list` (-l) each names a file of paths, one per line
std::vector<std::string> inputFiles(const std::vector<std::string> &args, size_t first, bool list);
// The pool / input arguments args[first..): "-" only in the first place, every other one a
// file that opens.  false after the message, which calls the arguments `word`s.
bool checkInputArguments(const std::vector<std::string> &args, size_t first, const char *word);
// A sketch reference fixes -k, -n, -a and -z: the message for each one given, with `dash`
// before the option's letter.  true where the run stops: at any of them (allStop), else at
// -k and -n only.
bool refuseSketchOptions(const Command &c, const char *dash, bool allStop);
// the reference is a sketch: k, s, seed, case and alphabet come from it
void inheritFromSketch(Parameters &p, const Sketch &reference);

// The k-mer size warning (CommandDistance.cpp:146-170, 327-331): the sequences of a sketch
// longer than p.warning allows, the longest named when the command ends.
struct KmerWarning {
    uint64_t lengthMax = 0;
    std::string lengthMaxName;
    double randomChance = 0;
    int kMin = 0, count = 0;
    void scan(const Sketch &sketch, const Parameters &p);
    void print(const Parameters &p, const Command &c) const;   // nothing in reads mode
};

}  // namespace fpmhost
